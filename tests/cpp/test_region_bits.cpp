// Host tool of tests/test_part_shapes_cpu.py (no GPU): what kh_codec.hpp itself gives for the
// numbers tests/part_shapes.py mirrors. Every argument "c<cap>" prints "cap rbits"
// (set_region_bits), every argument "k<K>" prints "K P R pad W KT" (make_params, kt_of).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "kh_codec.hpp"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        if (a[0] == 'c') {
            const uint64_t cap = std::strtoull(a + 1, nullptr, 10);
            kh::KParams p = kh::make_params(19);
            kh::set_region_bits(p, cap);
            std::printf("%llu %d\n", (unsigned long long)cap, p.rbits);
        } else if (a[0] == 'k') {
            const int K = std::atoi(a + 1);
            const kh::KParams p = kh::make_params(K);
            std::printf("%d %d %d %d %d %d\n", K, p.P, p.R, p.pad, p.W, kh::kt_of(K));
        } else {
            std::fprintf(stderr, "usage: %s c<cap> | k<K> ...\n", argv[0]);
            return 2;
        }
    }
    return 0;
}
