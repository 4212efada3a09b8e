// kh_strand.hip — the other strand: reads that come from the strand the contigs were not written in.
//   k_loc_text_rc        text -> uint64 per position: the index's value of rc(window) (the K bases in
//                        reverse order, each complemented), LOC_NONE = no window / absent / no value;
//                        + counts {windows, located}. k_loc_text's pass (kh_locate.hip) with
//                        text_key_rc (kh_text.hpp) in place of text_key.
//   k_seed_runs_strand   two position arrays (v: k_loc_text's, w: k_loc_text_rc's) + read offsets ->
//                        6 uint64 per read {start, value, run, strand, located forward, located
//                        reverse}; k_seed_runs' pass (kh_seed.hip) over four ballots.
// If rc(read[i .. i+K)) stands at contig position p, rc(read[i+1 .. i+1+K)) stands at p - 1: on the
// reverse strand a run's values go DOWN by one. i continues i-1 when both count, both are located and
// w[i-1] == w[i] + 1; the seed's value is w at the run's LAST window (its smallest), so on either
// strand the matched contig bytes are [value, value + run + K - 1).
// The lane states and loc_step are a copy of kh_locate.hip's, not a header shared with it: that file's
// kernels were to keep their code objects (as k_seed_cov's line_of, kh_seed.hip).
#include <hip/hip_runtime.h>

#include "kh_device.hpp"
#include "kh_kernels.hpp"
#include "kh_stage.hpp"
#include "kh_text.hpp"

namespace kh {

namespace {

// lane states of the query kernel (kh_locate.hip)
constexpr uint32_t LS_IDLE = 0, LS_PROBE = 1, LS_VALUE = 2;

// One iteration of the state machine (kh_locate.hip loc_step): a lane in LS_VALUE issues its loc load,
// every lane in LS_PROBE its quad_probe, then the value goes to vt[mine] and a hit becomes LS_VALUE.
// True when this lane's answer was a position.
template <int W>
__device__ __forceinline__ bool loc_step(uint32_t& st, uint64_t& s, uint64_t& pb, const Key& k, uint32_t mine,
                                         const uint64_t* __restrict__ slots, uint64_t cap,
                                         const uint64_t* __restrict__ loc, uint64_t pb_max, const KParams& p,
                                         uint32_t q, uint32_t ql, uint64_t* vt) {
    uint64_t v = LOC_NONE;
    if (st == LS_VALUE) v = __builtin_nontemporal_load(loc + s);  // s: the hit slot
    const QuadProbe pr = quad_probe<W>(st == LS_PROBE ? s : WQ_IDLE, k, slots, cap, nullptr, p, false, q, ql);
    if (st == LS_VALUE) {
        vt[mine] = v;
        st = LS_IDLE;
        return v != LOC_NONE;
    }
    if (st == LS_PROBE) {
        if (pr.fh < pr.fe) {
            s = (s & ~3ull) + pr.fh;
            st = LS_VALUE;
        } else if (pr.fe < 4u || ++pb > pb_max) {
            vt[mine] = LOC_NONE;
            st = LS_IDLE;
        } else {
            const uint64_t nx = (s & ~3ull) + 4;
            s = nx >= cap ? 0 : nx;
        }
    }
    return false;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Locate over text, reverse complement: k_loc_text with the key of rc(window idx).
template <int W>
__global__ __launch_bounds__(BLOCK) void k_loc_text_rc(KParams p, const uint8_t* __restrict__ text, uint64_t len,
                                                       const uint64_t* __restrict__ slots, uint64_t cap,
                                                       const uint64_t* __restrict__ loc, uint64_t* pos_out,
                                                       unsigned long long* counts) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[TX_RAW];
    __shared__ __attribute__((aligned(16))) uint64_t cw[TX_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t bw[TX_WORDS];
    __shared__ __attribute__((aligned(16))) uint64_t vtile[TEXT_TILE + 4];
    __shared__ uint32_t wsum[2 * (BLOCK / 64)];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane & 3u, ql = lane & ~3u;
    const uint64_t pb_max = (cap >> 2) + 2;
    const uint64_t ntiles = (len + TEXT_TILE - 1) / TEXT_TILE;
    constexpr uint32_t QUARTER = TEXT_TILE / (BLOCK / 64);
    uint32_t nwin = 0, nloc = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TEXT_TILE;
        const uint64_t left = len - base;
        const uint32_t cnt = left < (uint64_t)TEXT_TILE ? (uint32_t)left : (uint32_t)TEXT_TILE;
        const uint32_t halo = (uint32_t)TEXT_TILE + (uint32_t)p.K - 1u;
        const uint32_t nb = left < (uint64_t)halo ? (uint32_t)left : halo;
        __syncthreads();  // the last tile's answers have left
        const uint32_t a = stage_bytes(text + base, nb, raw);
        uint8_t* const vdst = pos_out ? reinterpret_cast<uint8_t*>(pos_out + base) : nullptr;
        const uint32_t va = (uint32_t)((uintptr_t)vdst & 15u);  // 0 or 8
        uint64_t* const vt = vtile + (va >> 3);
        __syncthreads();
        text_tile_codes(raw, a, nb, cw, bw);
        __syncthreads();
        const uint32_t w_hi = min(cnt, (wv + 1) * QUARTER);
        uint32_t nxt = wv * QUARTER;  // the wave's next position (uniform)
        uint32_t st = LS_IDLE, mine = 0;
        Key k{0, 0};
        uint64_t s = 0, pb = 0;
        while (true) {
            const uint64_t nm = __ballot(st == LS_IDLE);
            if (nm && nxt < w_hi) {
                const uint32_t idx = nxt + mbcnt64(nm);
                if (st == LS_IDLE && idx < w_hi) {
                    mine = idx;
                    if (text_valid(bw, idx, p)) {
                        k = text_key_rc<W>(cw, idx, p);
                        s = home_of(place(k, p), cap, p);
                        pb = 0;
                        st = LS_PROBE;
                        ++nwin;
                    } else {
                        vt[idx] = LOC_NONE;
                    }
                }
                nxt = min(w_hi, nxt + (uint32_t)__popcll(nm));
            }
            if (!__any(st != LS_IDLE)) {
                if (nxt >= w_hi) break;
                continue;  // a run of positions without windows: take the next ones
            }
            if (loc_step<W>(st, s, pb, k, mine, slots, cap, loc, pb_max, p, q, ql, vt)) ++nloc;
        }
        __syncthreads();
        if (vdst) flush_bytes(vdst, cnt * 8u, reinterpret_cast<const uint8_t*>(vtile), va);
    }
    if (!counts) return;  // uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nwin += __shfl_xor(nwin, o, 64);
        nloc += __shfl_xor(nloc, o, 64);
    }
    if (lane == 0) {
        wsum[2 * wv] = nwin;
        wsum[2 * wv + 1] = nloc;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long v = 0;
        for (uint32_t w = 0; w < BLOCK / 64; ++w) v += wsum[2 * w + threadIdx.x];
        if (v) atomicAdd(&counts[threadIdx.x], v);
    }
}

hipError_t launch_loc_text_rc(const KParams& p, const uint8_t* text, uint64_t len, TableView t, const uint64_t* loc,
                              uint64_t* pos_out, unsigned long long* counts, hipStream_t s) {
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, 16, s);
        if (e != hipSuccess) return e;
    }
    if (len == 0) return hipSuccess;
    const uint64_t ntiles = text_tiles(len);
    const unsigned grid = (unsigned)hmin(ntiles, (uint64_t)cu_count() * 8);
    with_w(p.W, [&](auto w) {
        k_loc_text_rc<decltype(w)::value><<<grid, BLOCK, 0, s>>>(p, text, len, t.slots, t.cap, loc, pos_out,
                                                                  counts);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The runs of one strand, all uniform: the best run {b_start, b_val, b_len} and the open one
// {o_start, o_val, o_len} (o_len = 0: none), as k_seed_runs keeps them. b_val / o_val are the value at
// the run's FIRST window on either strand.
struct StrandRuns {
    uint64_t b_start = 0, b_val = 0, b_len = 0;
    uint64_t o_start = 0, o_val = 0, o_len = 0;
};

// One chunk of 64 windows from c0 on for one strand (k_seed_runs' chunk step): x = this lane's value,
// locm / contm = the ballots of located and of "continues its left neighbour".
__device__ __forceinline__ void strand_chunk(StrandRuns& r, uint64_t x, uint64_t locm, uint64_t contm, uint64_t c0,
                                             uint32_t lane) {
    const uint64_t head = locm & ~contm;
    // the open run goes on through the ones at the bottom of cont
    const uint32_t t = ~contm ? (uint32_t)__builtin_ctzll(~contm) : 64u;
    if (t) {
        r.o_len += t;
        if (r.o_len > r.b_len) r.b_start = r.o_start, r.b_val = r.o_val, r.b_len = r.o_len;
    }
    // the runs that begin in this chunk; none of them is longer than 64
    if (head && r.b_len < 64) {
        uint32_t key = 0;  // (length, 63 - lane): the maximum is the longest, then the first
        if ((head >> lane) & 1ull) {
            const uint64_t above = (contm >> lane) >> 1;  // cont of the lanes above; bit 63 - lane is 0
            key = ((1u + (uint32_t)__builtin_ctzll(~above)) << 6) | (63u - lane);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, 64));
        const uint32_t l = key >> 6, h = 63u - (key & 63u);
        if ((uint64_t)l > r.b_len) r.b_start = c0 + h, r.b_val = __shfl(x, (int)h, 64), r.b_len = l;
    }
    // what stays open: lane 63 located -> the run of the topmost head, or the old one still going
    if (!(locm >> 63)) {
        r.o_len = 0;
    } else if (t < 64) {
        const uint32_t h = 63u - (uint32_t)__builtin_clzll(head);  // t < 64 and bit 63 located: a head exists
        r.o_start = c0 + h;
        r.o_val = __shfl(x, (int)h, 64);
        r.o_len = 64 - h;
    }
}

// One wave per read, 64 counted windows at a time: lane j loads v[c0 + j] and w[c0 + j]; the left
// neighbours come by a lane shift, lane 0's from the last chunk's lane 63 (uniform). Forward: v ==
// left + 1. Reverse: left == w + 1 (a left neighbour of 0 is never continued: 0 - 1 is LOC_NONE, and
// ...FFFE never continues LOC_NONE). Runs are met in ascending start and only a strictly longer one
// replaces the best, so a tie within a strand keeps the first; the forward best wins a tie between
// the strands.
__global__ __launch_bounds__(BLOCK) void k_seed_runs_strand(const uint64_t* __restrict__ pos_f,
                                                            const uint64_t* __restrict__ pos_r, uint64_t len,
                                                            const uint64_t* __restrict__ read_off, uint64_t n_reads,
                                                            uint32_t K, uint64_t* __restrict__ seeds) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6));
    const uint64_t nwaves = (uint64_t)gridDim.x * (BLOCK / 64);
    const uint64_t lim = min(len, read_off[n_reads]);  // nothing past the text or the last offset is read
    for (uint64_t r = wave0; r < n_reads; r += nwaves) {
        const uint64_t b = min(read_off[r], lim), e = min(read_off[r + 1], lim);
        const uint64_t nw = (e > b && e - b >= (uint64_t)K) ? e - b - K + 1 : 0;  // counted windows
        StrandRuns f, rv;
        uint64_t nloc_f = 0, nloc_r = 0;
        uint64_t last_v = LOC_NONE, last_w = LOC_NONE;
        for (uint64_t c0 = 0; c0 < nw; c0 += 64) {  // uniform
            const uint64_t i = c0 + lane;
            const uint64_t v = i < nw ? __builtin_nontemporal_load(pos_f + b + i) : LOC_NONE;
            const uint64_t w = i < nw ? __builtin_nontemporal_load(pos_r + b + i) : LOC_NONE;
            uint64_t left_v = __shfl_up(v, 1, 64), left_w = __shfl_up(w, 1, 64);
            if (lane == 0) left_v = last_v, left_w = last_w;
            const uint64_t loc_f = __ballot(v != LOC_NONE);
            const uint64_t cont_f = __ballot(v != LOC_NONE && left_v != LOC_NONE && v == left_v + 1);
            const uint64_t loc_r = __ballot(w != LOC_NONE);
            const uint64_t cont_r = __ballot(w != LOC_NONE && left_w != LOC_NONE && left_w == w + 1);
            nloc_f += (uint64_t)__popcll(loc_f);
            nloc_r += (uint64_t)__popcll(loc_r);
            strand_chunk(f, v, loc_f, cont_f, c0, lane);
            strand_chunk(rv, w, loc_r, cont_r, c0, lane);
            last_v = __shfl(v, 63, 64);
            last_w = __shfl(w, 63, 64);
        }
        // 48 bytes per read, 8-byte aligned only: lanes 0..5 store one word each
        if (lane < 6) {
            const bool rev = rv.b_len > f.b_len;  // equal runs: the forward one
            const uint64_t run = rev ? rv.b_len : f.b_len;
            const bool any = run != 0;
            const uint64_t start = rev ? rv.b_start : f.b_start;
            const uint64_t value = rev ? rv.b_val - (rv.b_len - 1) : f.b_val;  // reverse: w at the last window
            const uint64_t x = lane == 0 ? (any ? start : LOC_NONE)
                             : lane == 1 ? (any ? value : LOC_NONE)
                             : lane == 2 ? run
                             : lane == 3 ? (rev ? 1ull : 0ull)
                             : lane == 4 ? nloc_f : nloc_r;
            seeds[r * SEED_STRAND_WORDS + lane] = x;
        }
    }
}

hipError_t launch_seed_runs_strand(const uint64_t* pos_f, const uint64_t* pos_r, uint64_t len,
                                   const uint64_t* read_off, uint64_t n_reads, int K, uint64_t* seeds, hipStream_t s) {
    if (n_reads == 0) return hipSuccess;
    const uint64_t nb = (n_reads + BLOCK / 64 - 1) / (BLOCK / 64);
    const unsigned grid = (unsigned)hmin(nb, (uint64_t)cu_count() * 8);
    k_seed_runs_strand<<<grid, BLOCK, 0, s>>>(pos_f, pos_r, len, read_off, n_reads, (uint32_t)K, seeds);
    return hipGetLastError();
}

}  // namespace kh
