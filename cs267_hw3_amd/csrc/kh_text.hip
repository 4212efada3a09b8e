// kh_text.hip — find over text: every k-mer of a batch of sequences looked up on the device
// (hash_map.hpp:83-107 find, driven over read_kmers.hpp-style text instead of one packed key per
// call). Input is plain bytes: position i has a window iff bytes i .. i+K-1 lie in the text and are
// each one of A C G T; any other byte ('\n', 'N', lower case, 0, ...) ends the windows that cover it,
// so newline-separated contigs, reads and FASTA lines need no parsing.
//   k_find_text   text -> 2 bytes per position: {backward, forward} chars of the k-mer's record,
//                 {0, 0} = window present but k-mer absent, {0xFF, 0xFF} = no window; + counts
//   k_tk_count, k_tk_write   text -> the windows as pkmer_t keys + their positions, ascending (the
//                 sharded find answers text through them: dist.py find_text)
// A block works on a tile of TEXT_TILE positions: the tile's bytes plus a K-1 byte halo reach LDS
// through aligned 16-B loads (stage_bytes) and are turned ONCE into 2-bit codes (32 bases per 64-bit
// word, first base in the top bits: a window's V is a funnel shift of three words) and a bad-byte
// bitmap (one bit per byte, bytes past the end of the text are bad: "window at i" = no bad bit in
// [i, i + K), a shift and a mask of three words). No lane reads K bytes per position.
#include <hip/hip_runtime.h>

#include "kh_device.hpp"
#include "kh_kernels.hpp"
#include "kh_stage.hpp"
#include "kh_text.hpp"

namespace kh {

// ---------------------------------------------------------------------------------------------
// The fused pass: k_find_answer's per-lane state machine over the tile's positions instead of staged
// keys. Each wave works through its quarter of the tile; an idle lane takes the wave's next
// position (neighbouring lanes hold neighbouring k-mers, which share a minimizer for ~19 steps at
// k = 51 and so probe one placement region), a position without a window is answered at once, and
// every active lane issues ONE quad_probe per iteration. The answers are collected in LDS and leave
// as 16-B stores; windows and found are counted per lane and added once per block.
template <int W>
__global__ __launch_bounds__(BLOCK) void k_find_text(KParams p, const uint8_t* __restrict__ text, uint64_t len,
                                                     const uint64_t* __restrict__ slots, uint64_t cap,
                                                     uint8_t* ext_out, unsigned long long* counts) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[TX_RAW];
    __shared__ __attribute__((aligned(16))) uint64_t cw[TX_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t bw[TX_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t et[TEXT_TILE * 2 + 32];
    __shared__ uint32_t wsum[2 * (BLOCK / 64)];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane & 3u, ql = lane & ~3u;
    const uint64_t pb_max = (cap >> 2) + 2;  // every 4-slot block, the home block twice: absent (a full table)
    const uint64_t ntiles = (len + TEXT_TILE - 1) / TEXT_TILE;
    constexpr uint32_t QUARTER = TEXT_TILE / (BLOCK / 64);
    uint32_t nwin = 0, nfound = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TEXT_TILE;
        const uint64_t left = len - base;
        const uint32_t cnt = left < (uint64_t)TEXT_TILE ? (uint32_t)left : (uint32_t)TEXT_TILE;
        const uint32_t halo = (uint32_t)TEXT_TILE + (uint32_t)p.K - 1u;
        const uint32_t nb = left < (uint64_t)halo ? (uint32_t)left : halo;
        __syncthreads();  // the last tile's answers have left
        const uint32_t a = stage_bytes(text + base, nb, raw);
        uint8_t* const edst = ext_out ? ext_out + base * 2 : nullptr;
        const uint32_t ea = (uint32_t)((uintptr_t)edst & 15u);
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
                if (!active && idx < w_hi) {
                    mine = idx;
                    if (text_valid(bw, idx, p)) {
                        k = text_key(cw, idx, p);
                        s = home_of(place(k, p), cap, p);
                        pb = 0;
                        active = true;
                        ++nwin;
                    } else {
                        et[ea + 2u * idx] = 0xFF;  // KH_TEXT_NONE
                        et[ea + 2u * idx + 1u] = 0xFF;
                    }
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
                    const uint32_t e = pr.ext & 63u;
                    et[ea + 2u * mine] = code_char(ext_bwd(e));
                    et[ea + 2u * mine + 1u] = code_char(ext_fwd(e));
                    ++nfound;
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
        if (edst) flush_bytes(edst, cnt * 2u, et, ea);
    }
    if (!counts) return;  // uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nwin += __shfl_xor(nwin, o, 64);
        nfound += __shfl_xor(nfound, o, 64);
    }
    if (lane == 0) {
        wsum[2 * wv] = nwin;
        wsum[2 * wv + 1] = nfound;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long v = 0;
        for (uint32_t w = 0; w < BLOCK / 64; ++w) v += wsum[2 * w + threadIdx.x];
        if (v) atomicAdd(&counts[threadIdx.x], v);
    }
}

hipError_t launch_find_text(const KParams& p, const uint8_t* text, uint64_t len, TableView t, uint8_t* ext_out,
                            unsigned long long* counts, hipStream_t s) {
    if (counts) {
        hipError_t e = hipMemsetAsync(counts, 0, 16, s);
        if (e != hipSuccess) return e;
    }
    if (len == 0) return hipSuccess;
    const uint64_t ntiles = (len + TEXT_TILE - 1) / TEXT_TILE;
    const unsigned grid = (unsigned)hmin(ntiles, (uint64_t)cu_count() * 8);
    with_w(p.W, [&](auto w) {
        k_find_text<decltype(w)::value><<<grid, BLOCK, 0, s>>>(p, text, len, t.slots, t.cap, ext_out, counts);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Key extraction, two passes over the text with one block per tile: pass 1 counts the tile's
// windows, scan_exclusive turns the counts into offsets (and the total), pass 2 packs the tile's keys
// and positions into LDS in ascending position (a thread owns 8 consecutive positions; a block scan
// of the per-thread counts orders them) and stores them as consecutive 4-B words.
static constexpr int TX_PER = TEXT_TILE / BLOCK;  // positions per thread

struct TileCountF {
    const uint64_t* c;
    __device__ uint64_t operator()(uint64_t i) const { return c[i]; }
};

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_tk_pass(KParams p, const uint8_t* __restrict__ text, uint64_t len,
                                                   uint64_t* __restrict__ tile_cnt,
                                                   const uint64_t* __restrict__ tile_off, uint8_t* keys_out,
                                                   uint32_t* pos_out) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[TX_RAW];
    __shared__ __attribute__((aligned(16))) uint64_t cw[TX_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t bw[TX_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t sk[WRITE ? TEXT_TILE * TX_MAX_P : 16];
    __shared__ uint32_t spos[WRITE ? TEXT_TILE : 1];
    const uint32_t KP = (uint32_t)p.P;
    const uint64_t base = (uint64_t)blockIdx.x * TEXT_TILE;
    const uint64_t left = len - base;
    const uint32_t cnt = left < (uint64_t)TEXT_TILE ? (uint32_t)left : (uint32_t)TEXT_TILE;
    const uint32_t halo = (uint32_t)TEXT_TILE + (uint32_t)p.K - 1u;
    const uint32_t nb = left < (uint64_t)halo ? (uint32_t)left : halo;
    const uint32_t a = stage_bytes(text + base, nb, raw);
    __syncthreads();
    text_tile_codes(raw, a, nb, cw, bw);
    __syncthreads();
    const uint32_t i0 = threadIdx.x * TX_PER;
    uint32_t vmask = 0;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)TX_PER; ++j)
        if (i0 + j < cnt && text_valid(bw, i0 + j, p)) vmask |= 1u << j;
    uint64_t tot;
    uint32_t at = (uint32_t)block_excl_scan((uint64_t)__popc(vmask), tot);
    if (!WRITE) {
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
        return;
    }
    for (uint32_t j = 0; j < (uint32_t)TX_PER; ++j) {
        if (!((vmask >> j) & 1u)) continue;
        key_to_packed(text_key(cw, i0 + j, p), sk + at * KP, p);
        spos[at] = (uint32_t)(base + i0 + j);
        ++at;
    }
    __syncthreads();
    const uint64_t g0 = tile_off[blockIdx.x];
    const uint32_t total = (uint32_t)tot;
    for (uint32_t j = threadIdx.x; j < total; j += BLOCK) pos_out[g0 + j] = spos[j];
    if (total) copy_run(keys_out + g0 * KP, sk, total * KP);
}

hipError_t launch_text_keys(const KParams& p, const uint8_t* text, uint64_t len, uint64_t* tile_cnt,
                            uint64_t* tile_off, uint64_t* scratch, uint8_t* keys_out, uint32_t* pos_out,
                            unsigned long long* count_out, hipStream_t s) {
    if (len < (uint64_t)p.K) return count_out ? hipMemsetAsync(count_out, 0, 8, s) : hipSuccess;
    const uint64_t ntiles = text_tiles(len);
    k_tk_pass<false><<<(unsigned)ntiles, BLOCK, 0, s>>>(p, text, len, tile_cnt, nullptr, nullptr, nullptr);
    hipError_t e = scan_exclusive(TileCountF{tile_cnt}, ntiles, tile_off, scratch, (unsigned long long*)nullptr,
                                  count_out, s);
    if (e != hipSuccess) return e;
    if (keys_out && pos_out)
        k_tk_pass<true><<<(unsigned)ntiles, BLOCK, 0, s>>>(p, text, len, nullptr, tile_off, keys_out, pos_out);
    return hipGetLastError();
}

}  // namespace kh
