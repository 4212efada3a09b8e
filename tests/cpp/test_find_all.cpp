// kh::ShardedTable::find_all (include/cs267_hw3_amd/dist_hash_map.hpp), driven by
// tests/test_cpp_find_all.py (which compiles this file with -DKMER_LEN=<k>):
//   test_find_all <kmer_file> <P> <peers>   P ranks as threads on GPU 0 over kh::ThreadComm, with a
//        peer group (peers = 1) or without one (0). Every rank inserts its block of the file, then
//        all ranks call find_all together, each with its own shuffle of every k-mer of the file plus
//        absent keys (a present k-mer with one base changed, not in the file); at P >= 3 the last
//        rank asks nothing (n = 0). Expected records come from the parsed input, never from the table.
// Exit status 0 = pass; a failed check prints it and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "cs267_hw3_amd/hash_map.hpp"
#include "cs267_hw3_amd/read_kmers.hpp"

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <kmer_file> <P> <peers 0|1>\n", argv[0]);
        return 2;
    }
    const std::string fname = argv[1];
    const int P = atoi(argv[2]);
    const bool peers = atoi(argv[3]) != 0;
    const std::vector<kmer_pair> all = read_kmers(fname);
    const size_t n = all.size(), KP = sizeof(pkmer_t), R = sizeof(kmer_pair);
    std::map<std::string, kmer_pair> dict;  // key bytes -> record, from the input text
    for (const auto& k : all) dict[std::string(reinterpret_cast<const char*>(k.kmer.data), KP)] = k;
    // absent keys: base (i % K) of every 3rd k-mer replaced by the next base, unless that is in the file
    std::vector<pkmer_t> absent;
    for (size_t i = 0; i < n; i += 3) {
        std::string s = all[i].kmer_str();
        char& c = s[i % KMER_LEN];
        c = c == 'A' ? 'C' : c == 'C' ? 'G' : c == 'G' ? 'T' : 'A';
        const pkmer_t p(s);
        if (!dict.count(std::string(reinterpret_cast<const char*>(p.data), KP))) absent.push_back(p);
    }
    if (absent.empty()) {
        fprintf(stderr, "no absent keys\n");
        return 1;
    }
    kh::ThreadComm::Group group(P);
    std::vector<std::thread> th;
    std::vector<int> ok(P, 0);
    std::vector<size_t> asked(P, 0);
    for (int r = 0; r < P; ++r)
        th.emplace_back([&, r] {
            try {
                kh::hip_check(hipSetDevice(0), "hipSetDevice");
                const std::vector<kmer_pair> mine = read_kmers(fname, P, r);
                kh::ShardedTable st(KMER_LEN, n / P + 1, *group.comm(r), 0, peers ? &group : nullptr);
                st.insert_all(mine.data(), mine.size());
                std::vector<pkmer_t> q;
                if (!(P >= 3 && r == P - 1)) {
                    for (const auto& k : all) q.push_back(k.kmer);
                    q.insert(q.end(), absent.begin(), absent.end());
                    uint64_t x = 88172645463325252ull + (uint64_t)r;  // xorshift shuffle, one per rank
                    for (size_t i = q.size(); i > 1; --i) {
                        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                        std::swap(q[i - 1], q[x % i]);
                    }
                }
                std::vector<uint8_t> recs(q.size() * R + 1, 0xAB), found(q.size() + 1, 0xAB);
                st.find_all(reinterpret_cast<const uint8_t*>(q.data()), q.size(), recs.data(), found.data());
                int good = recs[q.size() * R] == 0xAB && found[q.size()] == 0xAB;  // nothing past the end
                size_t present = 0;
                for (size_t i = 0; i < q.size() && good; ++i) {
                    auto it = dict.find(std::string(reinterpret_cast<const char*>(q[i].data), KP));
                    uint8_t want[sizeof(kmer_pair)] = {0};
                    if (it != dict.end()) std::memcpy(want, &it->second, R), ++present;
                    good = found[i] == (it != dict.end() ? 1 : 0) && !std::memcmp(want, &recs[i * R], R);
                    if (!good) fprintf(stderr, "rank %d: key %zu: found %d\n", r, i, (int)found[i]);
                }
                if (!q.empty()) good = good && present == n;
                st.barrier();
                ok[r] = good;
                asked[r] = q.size();
            } catch (const std::exception& ex) {
                fprintf(stderr, "rank %d: %s\n", r, ex.what());
                group.abort();
            }
        });
    for (auto& t : th) t.join();
    for (int r = 0; r < P; ++r)
        if (!ok[r]) {
            fprintf(stderr, "rank %d: find_all differs from the input records\n", r);
            return 1;
        }
    printf("find_all ok: n=%zu absent=%zu P=%d peers=%d asked0=%zu\n", n, absent.size(), P, (int)peers, asked[0]);
    return 0;
}
