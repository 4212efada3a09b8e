// kh_locate.hip — the position index: one uint64 per table slot (loc[cap], all-ones = LOC_NONE = no
// position), beside the slots. It says where in the assembled contigs a k-mer sits: the slot of a hit
// is (s & ~3) + fh of its quad_probe, and loc[slot] holds the smallest position any build or set gave
// that k-mer.
//   k_loc_build   text -> atomicMin(loc[slot of the k-mer at i], base + i) for every window
//   k_loc_set     keys + a uint64 value each -> the same atomicMin; keys the table lacks are counted
//   k_loc_get     keys -> uint64 per key: loc[slot], LOC_NONE = absent or no value
//   k_loc_text    text -> uint64 per position, LOC_NONE = no window / absent / no value; + counts
//   k_loc_lines   text positions -> {line index, column} by binary search over the line starts
// The first four are k_find_text's / k_find_answer's shape: the same tile staging (kh_stage.hpp,
// kh_text.hpp), the same per-lane state machine with ONE quad_probe per active lane per iteration,
// outputs collected in LDS and stored as 16-B runs. A located key costs two dependent random requests
// (the slot block, then loc[slot]): the two query kernels give a lane a "value pending" state, in
// which it issues its loc load in the iteration where the other lanes probe, so the wave overlaps the
// two instead of running them one after the other.
#include <hip/hip_runtime.h>

#include "kh_device.hpp"
#include "kh_kernels.hpp"
#include "kh_stage.hpp"
#include "kh_text.hpp"

namespace kh {

static constexpr int LG_TILE = 4 * BLOCK;  // keys per block tile of the key kernels (256 per wave)

// lane states of the query kernels
static constexpr uint32_t LS_IDLE = 0, LS_PROBE = 1, LS_VALUE = 2;

// Smallest position wins: 64-bit, relaxed, agent scope, no return value (one vector atomic).
__device__ __forceinline__ void loc_min(unsigned long long* loc, uint64_t slot, uint64_t v) {
    (void)__hip_atomic_fetch_min(loc + slot, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------
// Build over text: k_find_text's pass with the atomic in place of the answer.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_loc_build(KParams p, const uint8_t* __restrict__ text, uint64_t len,
                                                     const uint64_t* __restrict__ slots, uint64_t cap,
                                                     unsigned long long* loc, uint64_t pos0) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[TX_RAW];
    __shared__ __attribute__((aligned(16))) uint64_t cw[TX_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t bw[TX_WORDS];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane & 3u, ql = lane & ~3u;
    const uint64_t pb_max = (cap >> 2) + 2;  // every 4-slot block, the home block twice: absent (a full table)
    const uint64_t ntiles = (len + TEXT_TILE - 1) / TEXT_TILE;
    constexpr uint32_t QUARTER = TEXT_TILE / (BLOCK / 64);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TEXT_TILE;
        const uint64_t left = len - base;
        const uint32_t cnt = left < (uint64_t)TEXT_TILE ? (uint32_t)left : (uint32_t)TEXT_TILE;
        const uint32_t halo = (uint32_t)TEXT_TILE + (uint32_t)p.K - 1u;
        const uint32_t nb = left < (uint64_t)halo ? (uint32_t)left : halo;
        __syncthreads();  // the last tile's codes are read
        const uint32_t a = stage_bytes(text + base, nb, raw);
        __syncthreads();
        text_tile_codes(raw, a, nb, cw, bw);
        __syncthreads();
        const uint32_t w_hi = min(cnt, (wv + 1) * QUARTER);
        uint32_t nxt = wv * QUARTER;  // the wave's next position (uniform)
        bool active = false;
        uint32_t mine = 0;
        Key k{0, 0};
        uint64_t s = 0, pb = 0;
        while (true) {
            const uint64_t nm = __ballot(!active);
            if (nm && nxt < w_hi) {
                const uint32_t idx = nxt + mbcnt64(nm);
                if (!active && idx < w_hi && text_valid(bw, idx, p)) {
                    mine = idx;
                    k = text_key(cw, idx, p);
                    s = home_of(place(k, p), cap, p);
                    pb = 0;
                    active = true;
                }
                nxt = min(w_hi, nxt + (uint32_t)__popcll(nm));
            }
            if (!__any(active)) {
                if (nxt >= w_hi) break;
                continue;  // a run of positions without windows: take the next ones
            }
            const QuadProbe pr = quad_probe<W>(active ? s : WQ_IDLE, k, slots, cap, nullptr, p, false, q, ql);
            if (active) {
                if (pr.fh < pr.fe) {
                    loc_min(loc, (s & ~3ull) + pr.fh, pos0 + base + mine);
                    active = false;
                } else if (pr.fe < 4u || ++pb > pb_max) {
                    active = false;  // a k-mer the table does not hold
                } else {
                    const uint64_t nx = (s & ~3ull) + 4;
                    s = nx >= cap ? 0 : nx;
                }
            }
        }
    }
}

hipError_t launch_loc_build(const KParams& p, const uint8_t* text, uint64_t len, TableView t, uint64_t* loc,
                            uint64_t pos0, hipStream_t s) {
    if (len < (uint64_t)p.K) return hipSuccess;
    const uint64_t ntiles = text_tiles(len);
    const unsigned grid = (unsigned)hmin(ntiles, (uint64_t)cu_count() * 8);
    with_w(p.W, [&](auto w) {
        k_loc_build<decltype(w)::value><<<grid, BLOCK, 0, s>>>(p, text, len, t.slots, t.cap,
                                                               (unsigned long long*)loc, pos0);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Set by keys: k_find_answer's pass; a hit takes the key's value (values is 8-byte aligned: a lane
// reads its own when it takes the key).
template <int W>
__global__ __launch_bounds__(BLOCK) void k_loc_set(KParams p, const uint8_t* __restrict__ keys, uint64_t m,
                                                   const uint64_t* __restrict__ values,
                                                   const uint64_t* __restrict__ slots, uint64_t cap,
                                                   unsigned long long* loc, unsigned long long* missing) {
    __shared__ __attribute__((aligned(16))) uint8_t kt[LG_TILE * TX_MAX_P + 32];
    __shared__ uint32_t wsum[BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane & 3u, ql = lane & ~3u;
    const uint32_t KP = (uint32_t)p.P;
    const uint64_t pb_max = (cap >> 2) + 2;
    const uint64_t ntiles = (m + LG_TILE - 1) / LG_TILE;
    uint32_t nmiss = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * LG_TILE;
        const uint32_t cnt = m - base < (uint64_t)LG_TILE ? (uint32_t)(m - base) : (uint32_t)LG_TILE;
        __syncthreads();  // the last tile's keys are parsed
        const uint32_t a = stage_bytes(keys + base * KP, cnt * KP, kt);
        __syncthreads();
        const uint32_t w_hi = min(cnt, (wv + 1) * (uint32_t)BLOCK);
        uint32_t nxt = wv * (uint32_t)BLOCK;  // the wave's next key (uniform)
        bool active = false;
        Key k{0, 0};
        uint64_t s = 0, pb = 0, val = 0;
        while (true) {
            const uint64_t nm = __ballot(!active);
            if (nm && nxt < w_hi) {
                const uint32_t idx = nxt + mbcnt64(nm);
                if (!active && idx < w_hi) {
                    k = key_from_packed(kt + a + idx * KP, p);
                    val = values[base + idx];
                    s = home_of(place(k, p), cap, p);
                    pb = 0;
                    active = true;
                }
                nxt = min(w_hi, nxt + (uint32_t)__popcll(nm));
            }
            if (!__any(active)) break;
            const QuadProbe pr = quad_probe<W>(active ? s : WQ_IDLE, k, slots, cap, nullptr, p, false, q, ql);
            if (active) {
                if (pr.fh < pr.fe) {
                    loc_min(loc, (s & ~3ull) + pr.fh, val);
                    active = false;
                } else if (pr.fe < 4u || ++pb > pb_max) {
                    ++nmiss;
                    active = false;
                } else {
                    const uint64_t nx = (s & ~3ull) + 4;
                    s = nx >= cap ? 0 : nx;
                }
            }
        }
    }
    if (!missing) return;  // uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmiss += __shfl_xor(nmiss, o, 64);
    if (lane == 0) wsum[wv] = nmiss;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long v = 0;
        for (uint32_t w = 0; w < BLOCK / 64; ++w) v += wsum[w];
        if (v) atomicAdd(missing, v);
    }
}

hipError_t launch_loc_set(const KParams& p, const uint8_t* keys, uint64_t m, const uint64_t* values, TableView t,
                          uint64_t* loc, unsigned long long* missing, hipStream_t s) {
    if (missing) {
        hipError_t e = hipMemsetAsync(missing, 0, 8, s);
        if (e != hipSuccess) return e;
    }
    if (m == 0) return hipSuccess;
    const uint64_t ntiles = (m + LG_TILE - 1) / LG_TILE;
    const unsigned grid = (unsigned)hmin(ntiles, (uint64_t)cu_count() * 8);
    with_w(p.W, [&](auto w) {
        k_loc_set<decltype(w)::value><<<grid, BLOCK, 0, s>>>(p, keys, m, values, t.slots, t.cap,
                                                             (unsigned long long*)loc, missing);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// One iteration of the two query kernels' state machine, after the idle lanes took their work: a
// lane in LS_VALUE issues its loc load, every lane in LS_PROBE its quad_probe (both are in flight
// together), then the value is stored to the answer tile vt[mine] and a hit becomes LS_VALUE. Returns
// true when this lane's answer was a position (not LOC_NONE).
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

// Locate by keys. The 8-byte answers of a tile are collected in LDS (pos_out is 8-byte aligned: the
// tile starts 0 or 8 bytes into a 16-B granule) and leave as 16-B stores.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_loc_get(KParams p, const uint8_t* __restrict__ keys, uint64_t m,
                                                   const uint64_t* __restrict__ slots, uint64_t cap,
                                                   const uint64_t* __restrict__ loc, uint64_t* pos_out) {
    __shared__ __attribute__((aligned(16))) uint8_t kt[LG_TILE * TX_MAX_P + 32];
    __shared__ __attribute__((aligned(16))) uint64_t vtile[LG_TILE + 4];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane & 3u, ql = lane & ~3u;
    const uint32_t KP = (uint32_t)p.P;
    const uint64_t pb_max = (cap >> 2) + 2;
    const uint64_t ntiles = (m + LG_TILE - 1) / LG_TILE;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * LG_TILE;
        const uint32_t cnt = m - base < (uint64_t)LG_TILE ? (uint32_t)(m - base) : (uint32_t)LG_TILE;
        __syncthreads();  // the last tile's answers have left
        const uint32_t a = stage_bytes(keys + base * KP, cnt * KP, kt);
        uint8_t* const vdst = reinterpret_cast<uint8_t*>(pos_out + base);
        const uint32_t va = (uint32_t)((uintptr_t)vdst & 15u);  // 0 or 8
        uint64_t* const vt = vtile + (va >> 3);
        __syncthreads();
        const uint32_t w_hi = min(cnt, (wv + 1) * (uint32_t)BLOCK);
        uint32_t nxt = wv * (uint32_t)BLOCK;  // the wave's next key (uniform)
        uint32_t st = LS_IDLE, mine = 0;
        Key k{0, 0};
        uint64_t s = 0, pb = 0;
        while (true) {
            const uint64_t nm = __ballot(st == LS_IDLE);
            if (nm && nxt < w_hi) {
                const uint32_t idx = nxt + mbcnt64(nm);
                if (st == LS_IDLE && idx < w_hi) {
                    mine = idx;
                    k = key_from_packed(kt + a + idx * KP, p);
                    s = home_of(place(k, p), cap, p);
                    pb = 0;
                    st = LS_PROBE;
                }
                nxt = min(w_hi, nxt + (uint32_t)__popcll(nm));
            }
            if (!__any(st != LS_IDLE)) break;
            loc_step<W>(st, s, pb, k, mine, slots, cap, loc, pb_max, p, q, ql, vt);
        }
        __syncthreads();
        flush_bytes(vdst, cnt * 8u, reinterpret_cast<const uint8_t*>(vtile), va);
    }
}

hipError_t launch_loc_get(const KParams& p, const uint8_t* keys, uint64_t m, TableView t, const uint64_t* loc,
                          uint64_t* pos_out, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const uint64_t ntiles = (m + LG_TILE - 1) / LG_TILE;
    const unsigned grid = (unsigned)hmin(ntiles, (uint64_t)cu_count() * 8);
    with_w(p.W, [&](auto w) {
        k_loc_get<decltype(w)::value><<<grid, BLOCK, 0, s>>>(p, keys, m, t.slots, t.cap, loc, pos_out);
    });
    return hipGetLastError();
}

// Locate over text: k_find_text's pass with the value-pending state; a tile's answers are 16 KB of LDS.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_loc_text(KParams p, const uint8_t* __restrict__ text, uint64_t len,
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
                        k = text_key(cw, idx, p);
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

hipError_t launch_loc_text(const KParams& p, const uint8_t* text, uint64_t len, TableView t, const uint64_t* loc,
                           uint64_t* pos_out, unsigned long long* counts, hipStream_t s) {
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, 16, s);
        if (e != hipSuccess) return e;
    }
    if (len == 0) return hipSuccess;
    const uint64_t ntiles = text_tiles(len);
    const unsigned grid = (unsigned)hmin(ntiles, (uint64_t)cu_count() * 8);
    with_w(p.W, [&](auto w) {
        k_loc_text<decltype(w)::value><<<grid, BLOCK, 0, s>>>(p, text, len, t.slots, t.cap, loc, pos_out, counts);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Positions to lines: the line of position x is the last one starting at or before x (off: nc line
// starts, ascending; *total: the text's bytes). LOC_NONE, a position past the text or no line at
// all: LOC_NONE for both.
__global__ __launch_bounds__(BLOCK) void k_loc_lines(const uint64_t* __restrict__ pos, uint64_t m,
                                                     const uint64_t* __restrict__ off, uint64_t nc,
                                                     const unsigned long long* __restrict__ total,
                                                     uint64_t* __restrict__ line_out, uint64_t* __restrict__ col_out) {
    const uint64_t bytes = nc ? *total : 0;
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < m; j += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t x = pos[j];
        uint64_t line = LOC_NONE, col = LOC_NONE;
        if (x < bytes) {  // LOC_NONE is never below
            uint64_t lo = 0, hi = nc;  // off[lo] <= x < off[hi] (off[0] = 0, off[nc] = bytes)
            while (hi - lo > 1) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (off[mid] <= x)
                    lo = mid;
                else
                    hi = mid;
            }
            line = lo;
            col = x - off[lo];
        }
        line_out[j] = line;
        col_out[j] = col;
    }
}

hipError_t launch_loc_lines(const uint64_t* pos, uint64_t m, const uint64_t* off, uint64_t nc,
                            const unsigned long long* total, uint64_t* line_out, uint64_t* col_out, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const uint64_t nb = (m + BLOCK - 1) / BLOCK;
    const unsigned grid = (unsigned)hmin(nb, (uint64_t)cu_count() * 16);
    k_loc_lines<<<grid, BLOCK, 0, s>>>(pos, m, off, nc, total, line_out, col_out);
    return hipGetLastError();
}

}  // namespace kh
