// kh_text.hpp — a tile of text in LDS, shared by the kernels that work over text (kh_text.hip: find
// over text, key extraction; kh_locate.hip: the position index's build and query; kh_strand.hip: the
// query of every window's reverse complement): the tile's bytes
// plus a K-1 byte halo are turned ONCE into 2-bit codes (32 bases per 64-bit word, first base in the
// top bits: a window's V is a funnel shift of three words) and a bad-byte bitmap (one bit per byte,
// bytes past the end of the text are bad: "window at i" = no bad bit in [i, i + K), a shift and a
// mask of three words). No lane reads K bytes per position.
#pragma once
#include <hip/hip_runtime.h>

#include "kh_device.hpp"
#include "kh_kernels.hpp"

namespace kh {

static constexpr int TX_WORDS = TEXT_TILE / 32 + 2;           // 32-base words a tile's windows reach into
static constexpr int TX_GROUPS = TX_WORDS * 4;                // 8-base groups (one per thread and round)
static constexpr int TX_RAW = (TEXT_TILE + KMAX - 1 + 32 + 15) & ~15;  // staged bytes (stage_bytes: + 32)
static constexpr int TX_MAX_P = 15;                           // K <= 60 -> PACKED <= 15
static_assert(TEXT_TILE % (4 * 32) == 0, "a wave's quarter of the tile is whole words");
static_assert(TX_WORDS * 32 >= TEXT_TILE + KMAX - 1, "the code words cover the halo");

// raw[a + j], j in [0, nb): the tile's bytes -> cw (codes) and bw (bad bits) for every base of the
// TX_WORDS words; bytes at j >= nb (past the text, or past the halo) are bad. A thread converts 8
// bases, 4 neighbouring lanes OR their pieces into one word. Whole block; barrier before and after.
__device__ __forceinline__ void text_tile_codes(const uint8_t* raw, uint32_t a, uint32_t nb, uint64_t* cw,
                                                uint32_t* bw) {
#pragma unroll
    for (uint32_t g0 = 0; g0 < (uint32_t)TX_GROUPS; g0 += BLOCK) {  // uniform: every lane shuffles
        const uint32_t g = g0 + threadIdx.x;
        uint32_t c16 = 0, b8 = 0;
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const uint32_t j = 8u * g + b;
            const uint32_t code = j < nb ? base_code(raw[a + j]) : EXT_BAD;
            c16 |= (code & 3u) << (14u - 2u * b);
            b8 |= (code > 3u ? 1u : 0u) << b;
        }
        uint64_t c = (uint64_t)c16 << (48u - 16u * (g & 3u));
        uint32_t d = b8 << (8u * (g & 3u));
        c |= __shfl_xor(c, 1, 64);
        d |= __shfl_xor(d, 1, 64);
        c |= __shfl_xor(c, 2, 64);
        d |= __shfl_xor(d, 2, 64);
        if ((g & 3u) == 0 && g < (uint32_t)TX_GROUPS) {
            cw[g >> 2] = c;
            bw[g >> 2] = d;
        }
    }
}

// window at tile position i (< TEXT_TILE)?
__device__ __forceinline__ bool text_valid(const uint32_t* bw, uint32_t i, const KParams& p) {
    const uint32_t q = i >> 5, r = i & 31u;
    uint64_t bits = ((uint64_t)bw[q] | ((uint64_t)bw[q + 1] << 32)) >> r;
    if (r) bits |= (uint64_t)bw[q + 2] << (64u - r);
    return (bits & ((1ull << p.K) - 1)) == 0;  // K <= 60
}

// its k-mer: the top 2K bits of the 192 code bits from base i on
__device__ __forceinline__ Key text_key(const uint64_t* cw, uint32_t i, const KParams& p) {
    const uint32_t q = i >> 5, s = 2u * (i & 31u);
    unsigned __int128 x = ((unsigned __int128)cw[q] << 64) | cw[q + 1];
    if (s) x = (x << s) | (cw[q + 2] >> (64u - s));
    x >>= 128 - 2 * p.K;
    Key k;
    k.lo = (uint64_t)x & LO_MASK;
    k.hi = (uint64_t)(x >> 62);
    return k;
}

// the k-mer of its reverse complement (the K bases in reverse order, each code ^ 3): the same funnel
// shift, complemented; reversing the 2-bit groups of the 128 bits (rev2_64 of the two halves, swapped)
// brings base 0 to bits 0-1 and base K-1 to the top of the low 2K bits, the bases after the window
// above them. W = 1 (K <= 29): the window lies in the top word, whose reversal is the whole key.
template <int W = 2>
__device__ __forceinline__ Key text_key_rc(const uint64_t* cw, uint32_t i, const KParams& p) {
    const uint32_t q = i >> 5, s = 2u * (i & 31u);
    unsigned __int128 x = ((unsigned __int128)cw[q] << 64) | cw[q + 1];
    if (s) x = (x << s) | (cw[q + 2] >> (64u - s));
    x = ~x;
    Key k;
    if constexpr (W == 1) {
        k.lo = rev2_64((uint64_t)(x >> 64)) & p.v_mask;
        k.hi = 0;
        return k;
    }
    unsigned __int128 r = ((unsigned __int128)rev2_64((uint64_t)x) << 64) | rev2_64((uint64_t)(x >> 64));
    r &= ((unsigned __int128)1 << (2 * p.K)) - 1;  // K <= 60
    k.lo = (uint64_t)r & LO_MASK;
    k.hi = (uint64_t)(r >> 62);
    return k;
}

}  // namespace kh
