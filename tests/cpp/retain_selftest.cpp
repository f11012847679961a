// The host arithmetic of retain (backuwup_amd/csrc/bw_retain_host.h) in a stand-alone program: the words
// of a root set, where a root's bit lies, the bits that name a root, the refusal of a foreign bit, the
// drop predicate, the forward order of a sweep, and the last word's valid bits at 63, 64, 65, 4095 and 4096
// roots with a foreign bit planted in the last row.  Every expected value is worked out by hand
// (tests/test_retain_host.py holds the output); built plain and under the address and undefined sanitizers.
#include <cstdio>
#include <vector>

#include "bw_retain_host.h"

using namespace bw;

int main() {
    {   // A: W
        std::printf("A %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)rt_words(0), (unsigned long long)rt_words(1),
                    (unsigned long long)rt_words(64), (unsigned long long)rt_words(65), (unsigned long long)rt_words(128),
                    (unsigned long long)rt_words(129), (unsigned long long)rt_words(RT_MAX_ROOTS));
    }
    {   // B: the place of a root's bit: entry 5 of W = 3
        std::printf("B %llu %llu %llu %llx %llx %llx\n", (unsigned long long)rt_word(5, 3, 0), (unsigned long long)rt_word(5, 3, 64),
                    (unsigned long long)rt_word(5, 3, 191), (unsigned long long)rt_bit(0), (unsigned long long)rt_bit(63),
                    (unsigned long long)rt_bit(129));
    }
    {   // C: the valid bits of a word
        std::printf("C %llx %llx %llx %llx %llx %llx\n", (unsigned long long)rt_valid(0, 0), (unsigned long long)rt_valid(1, 0),
                    (unsigned long long)rt_valid(63, 0), (unsigned long long)rt_valid(64, 0), (unsigned long long)rt_valid(65, 1),
                    (unsigned long long)rt_valid(65, 0));
    }
    {   // D: foreign bits.  65 roots, W = 2: bit 0 of the second word is root 64, bit 1 is nobody's
        const std::vector<uint64_t> ok = {~0ull, 1, 0, 0, 5, 1}, bad = {~0ull, 1, 0, 2, 5, 1};
        const std::vector<uint64_t> full = {~0ull, ~0ull}, one = {0, 1, 2};
        std::printf("D %lld %lld %lld %lld %lld %lld %lld\n", (long long)rt_foreign(ok.data(), 3, 2, 65), (long long)rt_foreign(bad.data(), 3, 2, 65),
                    (long long)rt_foreign(full.data(), 2, 1, 64), (long long)rt_foreign(full.data(), 2, 1, 63),
                    (long long)rt_foreign(one.data(), 3, 1, 0), (long long)rt_foreign(one.data(), 3, 1, 1), (long long)rt_foreign(nullptr, 0, 1, 0));
    }
    {   // E: the drop predicate, W = 2
        const uint64_t m[2] = {5, 1}, none[2] = {0, 0}, all[2] = {~0ull, ~0ull}, low[2] = {5, 0}, both[2] = {5, 1}, z[2] = {0, 0};
        std::printf("E %d %d %d %d %d %d %d\n", rt_live(m, none, 2), rt_live(m, all, 2), rt_live(m, low, 2), rt_live(m, both, 2),
                    rt_live(z, none, 2), rt_any(m, 2), rt_any(z, 2));
    }
    {   // F: four levels, the second appends nothing: a forward sweep, then impact's backward one over the same list
        ImLevels L;
        std::printf("F empty %zu\n", rt_sweep(L).size());
        L.close(5), L.close(5), L.close(12), L.close(13);
        for (const auto& r : rt_sweep(L)) std::printf("F range %llu %llu\n", (unsigned long long)r.first, (unsigned long long)r.second);
        std::printf("F backward first %llu\n", (unsigned long long)L.sweep().front().first);
    }
    {   // G: the last word at the edges of a word and of the limit.  Three rows with every valid bit set are clean;
        // then one bit in the last word of the last row: its top bit, and its lowest bit no root has (bit 0 where
        // the word is full).  Past the last word nothing is valid.
        const uint64_t ns[5] = {63, 64, 65, RT_MAX_ROOTS - 1, RT_MAX_ROOTS};
        for (uint64_t n : ns) {
            const uint64_t W = rt_words(n), last = rt_valid(n, W - 1);
            std::vector<uint64_t> rows(3 * W);
            for (uint64_t i = 0; i < 3; i++)
                for (uint64_t w = 0; w < W; w++) rows[i * W + w] = rt_valid(n, w);
            const long long clean = (long long)rt_foreign(rows.data(), 3, W, n);
            std::vector<uint64_t> top = rows, low = rows;
            top[3 * W - 1] |= 1ull << 63;
            low[3 * W - 1] |= last + 1 ? last + 1 : 1;
            std::printf("G %llu %llu %llx %llx %lld %lld %lld\n", (unsigned long long)n, (unsigned long long)W, (unsigned long long)last,
                        (unsigned long long)rt_valid(n, W), clean, (long long)rt_foreign(top.data(), 3, W, n),
                        (long long)rt_foreign(low.data(), 3, W, n));
        }
    }
    return 0;
}
