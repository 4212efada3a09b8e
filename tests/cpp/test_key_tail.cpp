// Host test of kh_codec.hpp key_tail_piece (the run-append path of both walkers): the m oldest of
// the last n bases of a key, base i at bits 2i, against a per-base loop over V = hi * 2^62 + lo
// (base i of a K-mer = bits 2(K-1-i) of V). Every n in 1..min(63, K-1) and every first piece
// m in 1..min(n, 32), 64 random keys per K: both sides of the 62-bit word boundary of V and the
// m = 32 mask.
#include <cstdint>
#include <cstdio>

#include "kh_codec.hpp"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    const int Ks[] = {19, 31, 51, 60};
    unsigned long long checked = 0;
    for (int K : Ks) {
        const kh::KParams p = kh::make_params(K);
        for (int t = 0; t < 64; ++t) {
            kh::Key k;
            k.lo = rnd() & kh::LO_MASK & p.v_mask;
            k.hi = rnd() & p.hi_mask;
            const unsigned __int128 V = ((unsigned __int128)k.hi << 62) | k.lo;
            const int nmax = K - 1 < 63 ? K - 1 : 63;
            for (int n = 1; n <= nmax; ++n)
                for (int m = 1; m <= (n < 32 ? n : 32); ++m) {
                    uint64_t want = 0;
                    for (int j = 0; j < m; ++j) {
                        const int i = K - n + j;  // j-th oldest of the last n bases
                        want |= (uint64_t)((V >> (2 * (K - 1 - i))) & 3u) << (2 * j);
                    }
                    const uint64_t got = kh::key_tail_piece(k, (uint32_t)n, (uint32_t)m);
                    if (got != want) {
                        std::printf("key_tail_piece K=%d n=%d m=%d hi=%016llx lo=%016llx: got %016llx want %016llx\n", K,
                                    n, m, (unsigned long long)k.hi, (unsigned long long)k.lo, (unsigned long long)got,
                                    (unsigned long long)want);
                        return 1;
                    }
                    ++checked;
                }
        }
    }
    std::printf("key_tail ok %llu\n", checked);
    return 0;
}
