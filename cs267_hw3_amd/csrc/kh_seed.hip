// kh_seed.hip — seeds: the consumer of the position index. A batch of reads over a position array
// (one uint64 per text byte, as k_loc_text writes it; LOC_NONE = not located) -> per read its longest
// run of windows whose values go up by one, and per contig line the coverage those seeds give.
//   k_seed_runs   positions + read offsets -> 4 uint64 per read {start in the read, value at the run's
//                 first window, run length in windows, located windows}; one wave per read
//   k_seed_cov    seeds -> reads_per_line[line] += 1, bases_per_line[line] += run + K - 1 (one thread
//                 per read: k_loc_lines' binary search, then two 64-bit atomics)
// Window i of read [b, e) counts when i + K <= e. i continues i-1 when both count, both are located and
// v[i] == v[i-1] + 1; a run is a maximal chain of continuations, the seed the longest run, the first
// one on a tie. No LDS, no scratch: a chunk's runs come from two ballots.
#include <hip/hip_runtime.h>

#include "kh_device.hpp"
#include "kh_kernels.hpp"

namespace kh {

// One wave walks a read's counted windows 64 at a time: lane j loads v[c0 + j] (512 contiguous bytes
// per wave and chunk). located = v != NONE; cont = located, the left neighbour located and
// v == left + 1, the left neighbour's value by a lane shift, lane 0's from the last chunk's lane 63
// (uniform `last`). A head (located, not cont) at lane h leads a run of 1 + the ones of cont above h.
// The run that reaches lane 63 stays open as uniform {o_start, o_val, o_len} and grows by the ones at
// the bottom of the next chunk's cont. The best run is uniform {b_start, b_val, b_len}: runs are met
// in ascending start, and only a strictly longer one replaces it, so ties keep the smallest start.
__global__ __launch_bounds__(BLOCK) void k_seed_runs(const uint64_t* __restrict__ pos, uint64_t len,
                                                     const uint64_t* __restrict__ read_off, uint64_t n_reads,
                                                     uint32_t K, uint64_t* __restrict__ seeds) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6));
    const uint64_t nwaves = (uint64_t)gridDim.x * (BLOCK / 64);
    const uint64_t lim = min(len, read_off[n_reads]);  // nothing past the text or the last offset is read
    for (uint64_t r = wave0; r < n_reads; r += nwaves) {
        const uint64_t b = min(read_off[r], lim), e = min(read_off[r + 1], lim);
        const uint64_t nw = (e > b && e - b >= (uint64_t)K) ? e - b - K + 1 : 0;  // counted windows
        uint64_t b_start = 0, b_val = 0, b_len = 0, nloc = 0;
        uint64_t o_start = 0, o_val = 0, o_len = 0;  // the open run (o_len = 0: none)
        uint64_t last = LOC_NONE;
        for (uint64_t c0 = 0; c0 < nw; c0 += 64) {  // uniform
            const uint64_t i = c0 + lane;
            const uint64_t v = i < nw ? __builtin_nontemporal_load(pos + b + i) : LOC_NONE;
            uint64_t left = __shfl_up(v, 1, 64);
            if (lane == 0) left = last;
            const bool located = v != LOC_NONE;
            const uint64_t locm = __ballot(located);
            const uint64_t contm = __ballot(located && left != LOC_NONE && v == left + 1);
            const uint64_t head = locm & ~contm;
            nloc += (uint64_t)__popcll(locm);
            // the open run goes on through the ones at the bottom of cont (bit 0 set: lane 63 of the last
            // chunk was located, so a run is open)
            const uint32_t t = ~contm ? (uint32_t)__builtin_ctzll(~contm) : 64u;
            if (t) {
                o_len += t;
                if (o_len > b_len) b_start = o_start, b_val = o_val, b_len = o_len;
            }
            // the runs that begin in this chunk; none of them is longer than 64
            if (head && b_len < 64) {
                uint32_t key = 0;  // (length, 63 - lane): the maximum is the longest, then the first
                if ((head >> lane) & 1ull) {
                    const uint64_t above = (contm >> lane) >> 1;  // cont of the lanes above; bit 63 - lane is 0
                    key = ((1u + (uint32_t)__builtin_ctzll(~above)) << 6) | (63u - lane);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, 64));
                const uint32_t l = key >> 6, h = 63u - (key & 63u);
                if ((uint64_t)l > b_len) b_start = c0 + h, b_val = __shfl(v, (int)h, 64), b_len = l;
            }
            // what stays open: lane 63 located -> the run of the topmost head, or the old one still going
            if (!(locm >> 63)) {
                o_len = 0;
            } else if (t < 64) {
                const uint32_t h = 63u - (uint32_t)__builtin_clzll(head);  // t < 64 and bit 63 located: a head exists
                o_start = c0 + h;
                o_val = __shfl(v, (int)h, 64);
                o_len = 64 - h;
            }
            last = __shfl(v, 63, 64);
        }
        // 32 bytes per read, 8-byte aligned only (seeds may start 8 bytes into a 16-B granule): lanes
        // 0..3 store one word each, one instruction and one 32-byte request per read
        if (lane < 4) {
            const bool any = b_len != 0;
            const uint64_t w = lane == 0 ? (any ? b_start : LOC_NONE)
                             : lane == 1 ? (any ? b_val : LOC_NONE)
                             : lane == 2 ? b_len : nloc;
            seeds[r * 4 + lane] = w;
        }
    }
}

hipError_t launch_seed_runs(const uint64_t* pos, uint64_t len, const uint64_t* read_off, uint64_t n_reads, int K,
                            uint64_t* seeds, hipStream_t s) {
    if (n_reads == 0) return hipSuccess;
    const uint64_t nb = (n_reads + BLOCK / 64 - 1) / (BLOCK / 64);
    const unsigned grid = (unsigned)hmin(nb, (uint64_t)cu_count() * 8);
    k_seed_runs<<<grid, BLOCK, 0, s>>>(pos, len, read_off, n_reads, (uint32_t)K, seeds);
    return hipGetLastError();
}

// The line of text position x < the text's bytes over nc ascending line starts: k_loc_lines' search. A
// copy, not a helper shared with kh_locate.hip: calling one from k_loc_lines reorders two instructions
// of that kernel, and its code object was to stay as it is.
__device__ __forceinline__ uint64_t line_of(const uint64_t* __restrict__ off, uint64_t nc, uint64_t x) {
    uint64_t lo = 0, hi = nc;  // off[lo] <= x < off[hi] (off[0] = 0, off[nc] = the text's bytes)
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Coverage per contig line: a seed {., value, run, .} with run > 0 and its value inside the text adds
// one read and run + K - 1 bases to the value's line. Either array may be null (uniform).
__global__ __launch_bounds__(BLOCK) void k_seed_cov(const uint64_t* __restrict__ seeds, uint64_t n_reads,
                                                    const uint64_t* __restrict__ off, uint64_t nc,
                                                    const unsigned long long* __restrict__ total, uint32_t K,
                                                    unsigned long long* reads_per_line,
                                                    unsigned long long* bases_per_line) {
    const uint64_t bytes = nc ? *total : 0;
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; r < n_reads; r += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t v = seeds[r * 4 + 1], run = seeds[r * 4 + 2];
        if (run == 0 || v >= bytes) continue;  // LOC_NONE is never below
        const uint64_t line = line_of(off, nc, v);
        if (reads_per_line) atomicAdd(reads_per_line + line, 1ull);
        if (bases_per_line) atomicAdd(bases_per_line + line, (unsigned long long)(run + K - 1));
    }
}

hipError_t launch_seed_cov(const uint64_t* seeds, uint64_t n_reads, const uint64_t* off, uint64_t nc,
                           const unsigned long long* total, int K, uint64_t* reads_per_line,
                           uint64_t* bases_per_line, hipStream_t s) {
    if (n_reads == 0) return hipSuccess;
    const uint64_t nb = (n_reads + BLOCK - 1) / BLOCK;
    const unsigned grid = (unsigned)hmin(nb, (uint64_t)cu_count() * 16);
    k_seed_cov<<<grid, BLOCK, 0, s>>>(seeds, n_reads, off, nc, total, (uint32_t)K,
                                      (unsigned long long*)reads_per_line, (unsigned long long*)bases_per_line);
    return hipGetLastError();
}

}  // namespace kh
