// kh_find.hip — batched find across shards (hash_map.hpp:83-107 DistributedHashMap::find, any key
// from any rank), the key side of the sharded path:
//   asker:  k_fr_own + k_fr_scatter   keys -> keys grouped by owner rank + their original positions
//   owner:  k_find_answer             keys -> 2 bytes per key {backward, forward}, {0,0} = absent
//   asker:  k_fg_scatter + k_fg_emit  answers in grouped order -> kmer_pair records + found flags in
//                                     the caller's order (the bytes k_find writes on one table)
// Keys are PACKED (5 / 13 / up to 15) bytes each, unaligned for per-lane loads: every kernel stages a
// block's keys through LDS with aligned 16-B loads and parses them there, and every output tile is
// built in LDS and leaves as 16-B (records, answers, flags) or 4-B (owner runs, positions) stores
// of consecutive addresses.
#include <hip/hip_runtime.h>

#include "kh_device.hpp"
#include "kh_kernels.hpp"
#include "kh_stage.hpp"

namespace kh {

static constexpr int MAX_P = 15;        // K <= 60 -> PACKED <= 15
static constexpr int FA_TILE = 4 * BLOCK;  // keys per block tile of the answer kernel (256 per wave)

// ---------------------------------------------------------------------------------------------
// Route pass 1: owner of every key (kept for pass 2) + the block's owner histogram.
__global__ __launch_bounds__(BLOCK) void k_fr_own(KParams p, const uint8_t* __restrict__ keys, uint64_t n,
                                                  uint32_t P, uint32_t* __restrict__ own, uint64_t* hist) {
    __shared__ uint32_t h[MAX_RANKS];
    __shared__ __attribute__((aligned(16))) uint8_t st[BLOCK * MAX_P + 32];
    for (uint32_t q = threadIdx.x; q < P; q += BLOCK) h[q] = 0;
    const uint64_t b0 = (uint64_t)blockIdx.x * ROUTE_TILE;
    for (uint32_t j = 0; j < ROUTE_TILE / BLOCK; ++j) {
        const uint64_t sub = b0 + (uint64_t)j * BLOCK;
        if (sub >= n) break;  // uniform
        const uint32_t cnt = n - sub < (uint64_t)BLOCK ? (uint32_t)(n - sub) : (uint32_t)BLOCK;
        __syncthreads();  // the last sub-tile's keys are parsed (and h is zeroed)
        const uint32_t a = stage_bytes(keys + sub * (uint64_t)p.P, cnt * (uint32_t)p.P, st);
        __syncthreads();
        if (threadIdx.x < cnt) {
            const Key k = key_from_packed(st + a + threadIdx.x * p.P, p);
            const uint32_t q = owner_key(k, p, P);
            own[sub + threadIdx.x] = q;
            atomicAdd(&h[q], 1u);
        }
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < P; q += BLOCK) hist[(uint64_t)blockIdx.x * P + q] = h[q];
}

// Route pass 2: the block's keys sorted by owner in LDS, then each (block, owner) run leaves for its
// place in the owner's group (off) as consecutive bytes, and the keys' original positions with it.
__global__ __launch_bounds__(BLOCK) void k_fr_scatter(KParams p, const uint8_t* __restrict__ keys, uint64_t n,
                                                      uint32_t P, const uint32_t* __restrict__ own,
                                                      const uint64_t* __restrict__ hist,
                                                      const uint64_t* __restrict__ off, uint64_t nb,
                                                      uint8_t* keys_out, uint32_t* index_out) {
    __shared__ uint32_t h[MAX_RANKS], lbase[MAX_RANKS + 1];
    __shared__ uint64_t gbase[MAX_RANKS];
    __shared__ __attribute__((aligned(16))) uint8_t st[BLOCK * MAX_P + 32];
    __shared__ __attribute__((aligned(16))) uint8_t sk[ROUTE_TILE * MAX_P];
    __shared__ uint32_t sidx[ROUTE_TILE];
    __shared__ uint8_t sown[ROUTE_TILE];
    const uint32_t KP = (uint32_t)p.P;
    const uint64_t b0 = (uint64_t)blockIdx.x * ROUTE_TILE;
    if (threadIdx.x < 64) {  // wave 0: exclusive scan of the block's histogram (P <= 64)
        const uint32_t q = threadIdx.x;
        const uint32_t c = q < P ? (uint32_t)hist[(uint64_t)blockIdx.x * P + q] : 0u;
        uint32_t x = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if ((int)q >= o) x += y;
        }
        if (q < P) {
            lbase[q] = x - c;
            gbase[q] = off[(uint64_t)q * nb + blockIdx.x];
            h[q] = 0;
        }
        if (q == P - 1) lbase[P] = x;
    }
    for (uint32_t j = 0; j < ROUTE_TILE / BLOCK; ++j) {
        const uint64_t sub = b0 + (uint64_t)j * BLOCK;
        if (sub >= n) break;  // uniform
        const uint32_t cnt = n - sub < (uint64_t)BLOCK ? (uint32_t)(n - sub) : (uint32_t)BLOCK;
        __syncthreads();
        const uint32_t a = stage_bytes(keys + sub * (uint64_t)KP, cnt * KP, st);
        __syncthreads();
        if (threadIdx.x < cnt) {
            uint32_t q = own[sub + threadIdx.x];
            if (q >= P) q = P - 1;  // never (pass 1 wrote it); keeps every LDS index in range
            uint32_t lp = lbase[q] + atomicAdd(&h[q], 1u);
            if (lp >= (uint32_t)ROUTE_TILE) lp = ROUTE_TILE - 1;  // never
            const uint8_t* s = st + a + threadIdx.x * KP;
            uint8_t* d = sk + lp * KP;
            for (uint32_t b = 0; b < KP; ++b) d[b] = s[b];
            sidx[lp] = (uint32_t)(sub + threadIdx.x);
            sown[lp] = (uint8_t)q;
        }
    }
    __syncthreads();
    const uint32_t total = lbase[P];
    for (uint32_t j = threadIdx.x; j < total; j += BLOCK) {
        const uint32_t q = sown[j];
        index_out[gbase[q] + (j - lbase[q])] = sidx[j];
    }
    for (uint32_t q = 0; q < P; ++q) {  // uniform
        const uint32_t c = lbase[q + 1] - lbase[q];
        if (c) copy_run(keys_out + gbase[q] * KP, sk + lbase[q] * KP, c * KP);
    }
}

hipError_t launch_find_route(const KParams& p, const uint8_t* keys, uint64_t n, uint32_t nranks, uint64_t* hist,
                             uint64_t* off, uint64_t* scratch, uint32_t* own, uint8_t* keys_out, uint32_t* index_out,
                             uint64_t* counts, hipStream_t s) {
    unsigned long long* total = reinterpret_cast<unsigned long long*>(scratch);
    const uint64_t nb = route_blocks(n);
    if (nb == 0) return hipMemsetAsync(counts, 0, (nranks + 1) * 8, s);
    k_fr_own<<<(unsigned)nb, BLOCK, 0, s>>>(p, keys, n, nranks, own, hist);
    hipError_t e = scan_exclusive(HistF{hist, nb, nranks}, nb * nranks, off, scratch + 1,
                                  (unsigned long long*)nullptr, total, s);
    if (e != hipSuccess) return e;
    k_route_counts<0><<<1, MAX_RANKS, 0, s>>>(off, nb, nranks, total, counts);
    k_fr_scatter<<<(unsigned)nb, BLOCK, 0, s>>>(p, keys, n, nranks, own, hist, off, nb, keys_out, index_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Answer: a dependent random table load per key, in the walkers' shape. A block stages FA_TILE keys;
// each wave works through its quarter with a per-lane state machine: ONE quad_probe (one 4-slot
// block load) per lane per iteration, and a lane whose key is answered takes the wave's next key on
// the next iteration instead of waiting for the longest probe run among the 64. The 2-byte answers
// are collected in LDS and leave as one run of 16-B stores per tile.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_find_answer(KParams p, const uint8_t* __restrict__ keys, uint64_t m,
                                                       const uint64_t* __restrict__ slots, uint64_t cap,
                                                       uint8_t* ext_out) {
    __shared__ __attribute__((aligned(16))) uint8_t kt[FA_TILE * MAX_P + 32];
    __shared__ __attribute__((aligned(16))) uint8_t et[FA_TILE * 2 + 32];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane & 3u, ql = lane & ~3u;
    const uint32_t KP = (uint32_t)p.P;
    const uint64_t pb_max = (cap >> 2) + 2;  // every 4-slot block, the home block twice: absent (a full table)
    const uint64_t ntiles = (m + FA_TILE - 1) / FA_TILE;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * FA_TILE;
        const uint32_t cnt = m - base < (uint64_t)FA_TILE ? (uint32_t)(m - base) : (uint32_t)FA_TILE;
        __syncthreads();  // the last tile's answers have left
        const uint32_t a = stage_bytes(keys + base * KP, cnt * KP, kt);
        uint8_t* const edst = ext_out + base * 2;
        const uint32_t ea = (uint32_t)((uintptr_t)edst & 15u);
        __syncthreads();
        const uint32_t w_hi = min(cnt, (wv + 1) * (uint32_t)BLOCK);
        uint32_t nxt = wv * (uint32_t)BLOCK;  // the wave's next key (uniform)
        bool active = false;
        uint32_t mine = 0;
        Key k{0, 0};
        uint64_t s = 0, pb = 0;
        while (true) {
            const uint64_t nm = __ballot(!active);
            if (nm && nxt < w_hi) {
                const uint32_t idx = nxt + mbcnt64(nm);
                if (!active && idx < w_hi) {
                    mine = idx;
                    k = key_from_packed(kt + a + idx * KP, p);
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
                    const uint32_t e = pr.ext & 63u;
                    et[ea + 2u * mine] = code_char(ext_bwd(e));
                    et[ea + 2u * mine + 1u] = code_char(ext_fwd(e));
                    active = false;
                } else if (pr.fe < 4u || ++pb > pb_max) {
                    et[ea + 2u * mine] = 0;
                    et[ea + 2u * mine + 1u] = 0;
                    active = false;
                } else {
                    const uint64_t nx = (s & ~3ull) + 4;
                    s = nx >= cap ? 0 : nx;
                }
            }
        }
        __syncthreads();
        flush_bytes(edst, cnt * 2u, et, ea);
    }
}

hipError_t launch_find_answer(const KParams& p, const uint8_t* keys, uint64_t m, TableView t, uint8_t* ext_out,
                              hipStream_t s) {
    if (m == 0) return hipSuccess;
    const uint64_t ntiles = (m + FA_TILE - 1) / FA_TILE;
    const unsigned grid = (unsigned)hmin(ntiles, (uint64_t)cu_count() * 8);
    with_w(p.W, [&](auto w) {
        k_find_answer<decltype(w)::value><<<grid, BLOCK, 0, s>>>(p, keys, m, t.slots, t.cap, ext_out);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Gather pass 1: the answer of grouped key j belongs to the caller's key index[j].
__global__ __launch_bounds__(BLOCK) void k_fg_scatter(const uint32_t* __restrict__ index,
                                                      const uint8_t* __restrict__ ext, uint64_t n,
                                                      uint16_t* __restrict__ ext_orig) {
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t i = index[j];
        if (i < n) ext_orig[i] = (uint16_t)((uint32_t)ext[2 * j] | ((uint32_t)ext[2 * j + 1] << 8));
    }
}

// Gather pass 2: a tile of the caller's keys + their answers -> the tile's records and found flags
// built in LDS (write_record's bytes; an absent key's record is zeroed), stored whole.
__global__ __launch_bounds__(BLOCK) void k_fg_emit(KParams p, const uint8_t* __restrict__ keys, uint64_t n,
                                                   const uint16_t* __restrict__ ext_orig, uint8_t* recs_out,
                                                   uint8_t* found_out) {
    __shared__ __attribute__((aligned(16))) uint8_t kt[BLOCK * MAX_P + 32];
    __shared__ __attribute__((aligned(16))) uint8_t rt[BLOCK * MAX_R + 32];
    __shared__ __attribute__((aligned(16))) uint8_t ft[BLOCK + 32];
    const uint32_t KP = (uint32_t)p.P, R = (uint32_t)p.R;
    const uint64_t ntiles = (n + BLOCK - 1) / BLOCK;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * BLOCK;
        const uint32_t cnt = n - base < (uint64_t)BLOCK ? (uint32_t)(n - base) : (uint32_t)BLOCK;
        __syncthreads();  // the last tile's records have left
        const uint32_t a = stage_bytes(keys + base * KP, cnt * KP, kt);
        uint8_t* const rdst = recs_out + base * R;
        uint8_t* const fdst = found_out + base;
        const uint32_t ra = (uint32_t)((uintptr_t)rdst & 15u), fa = (uint32_t)((uintptr_t)fdst & 15u);
        const uint32_t e = threadIdx.x < cnt ? ext_orig[base + threadIdx.x] : 0u;
        __syncthreads();
        if (threadIdx.x < cnt) {
            uint8_t* o = rt + ra + threadIdx.x * R;
            if (e) {
                key_to_packed(key_from_packed(kt + a + threadIdx.x * KP, p), o, p);
                o[KP] = (uint8_t)e;
                o[KP + 1] = (uint8_t)(e >> 8);
            } else {
                for (uint32_t b = 0; b < R; ++b) o[b] = 0;
            }
            ft[fa + threadIdx.x] = e ? 1 : 0;
        }
        __syncthreads();
        flush_bytes(rdst, cnt * R, rt, ra);
        flush_bytes(fdst, cnt, ft, fa);
    }
}

hipError_t launch_find_gather(const KParams& p, const uint8_t* keys, uint64_t n, const uint32_t* index,
                              const uint8_t* ext_grouped, uint16_t* ext_orig, uint8_t* recs_out, uint8_t* found_out,
                              hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t nb = (n + BLOCK - 1) / BLOCK;
    const unsigned grid = (unsigned)hmin(nb, (uint64_t)cu_count() * 16);
    k_fg_scatter<<<grid, BLOCK, 0, s>>>(index, ext_grouped, n, ext_orig);
    k_fg_emit<<<grid, BLOCK, 0, s>>>(p, keys, n, ext_orig, recs_out, found_out);
    return hipGetLastError();
}

}  // namespace kh
