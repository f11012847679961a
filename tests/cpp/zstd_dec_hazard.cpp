// zstd_dec_hazard.cpp -- the decoder core (backuwup_amd/csrc/bw_zstd_dec_core.h) on the host under
// an execution policy that checks zd::Hazard, the rule by which the kernel's WaveExec decides
// whether a match waits at a barrier for the wave's earlier stores (bw_zstd_dec.hip).  The policy
// keeps, per output byte, whether it was stored since the last barrier, asks the same Hazard the
// kernel asks, and counts where the rule and the bytes disagree:
//   unsynced_reads  matches that did not wait although their source holds a byte stored since the
//                   last barrier (on the device: a read of bytes that may not have landed)
//   needless_waits  matches that waited although their source holds no such byte
//   waits           matches that waited
// Built by tests/test_zstd_plant.py with -fsanitize=address,undefined.
//
//   zstd_dec_hazard IN OUT
// IN:  u32 n, then per case u32 src_len, u32 dst_cap, src bytes.
// OUT: per case i32 error (zd::Err), u32 out_len, u32 waits, u32 unsynced_reads, u32 needless_waits,
//      out bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../backuwup_amd/csrc/bw_zstd_dec_core.h"

struct CheckExec {
    zd::Hazard hz{nullptr};
    const uint8_t* base;
    std::vector<uint8_t> fresh;  // per output byte: stored since the last barrier
    size_t lo, hi;               // the range of fresh that may hold a 1
    uint32_t waits = 0, unsynced_reads = 0, needless_waits = 0;

    CheckExec(const uint8_t* dst, size_t cap) : base(dst), fresh(cap, 0), lo(cap), hi(0) {}
    template <class F>
    void for_streams(uint32_t n, F f) {
        for (uint32_t k = 0; k < n; k++) f(k);
    }
    int any(int v) { return v; }
    void sync() {
        if (lo < hi) memset(fresh.data() + lo, 0, hi - lo);
        lo = fresh.size();
        hi = 0;
        hz.synced();
    }
    void stored(const uint8_t* d, uint32_t n) {
        const size_t at = (size_t)(d - base);
        memset(fresh.data() + at, 1, n);
        if (at < lo) lo = at;
        if (at + n > hi) hi = at + n;
    }
    void copy(uint8_t* d, const uint8_t* s, uint32_t n) {
        hz.wrote(d);
        memcpy(d, s, n);
        stored(d, n);
    }
    void fill(uint8_t* d, uint8_t b, uint32_t n) {
        hz.wrote(d);
        memset(d, b, n);
        stored(d, n);
    }
    void match(uint8_t* d, size_t off, uint32_t n) {
        const uint8_t* s = d - off;
        const size_t span = off < n ? off : n, at = (size_t)(s - base);
        bool touches = false;
        for (size_t i = 0; i < span; i++) touches |= fresh[at + i] != 0;
        if (hz.must_wait(d, off, n)) {
            waits++;
            needless_waits += !touches;
            sync();
        } else {
            unsynced_reads += touches;
        }
        hz.wrote(d);
        for (uint32_t i = 0; i < n; i++) d[i] = s[i];
        stored(d, n);
    }
};

static bool read_u32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        perror("open");
        return 2;
    }
    uint32_t n = 0;
    if (!read_u32(in, &n)) return 2;
    zd::State* st = new zd::State;
    zd::Scratch* sc = new zd::Scratch;
    uint8_t* lit = (uint8_t*)malloc(zd::BLOCK_MAX + zd::LIT_SLACK);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len = 0, cap = 0;
        if (!read_u32(in, &len) || !read_u32(in, &cap)) return 2;
        std::vector<uint8_t> src(len ? len : 1), dst(cap ? cap : 1, 0xEE);
        if (len && fread(src.data(), 1, len, in) != len) return 2;
        size_t got = 0;
        CheckExec x(dst.data(), cap);
        const int32_t e = zd::decode_frame(src.data(), len, dst.data(), cap, st, sc, lit, &got, x);
        const uint32_t head[4] = {(uint32_t)got, x.waits, x.unsynced_reads, x.needless_waits};
        fwrite(&e, 4, 1, out);
        fwrite(head, 4, 4, out);
        if (got) fwrite(dst.data(), 1, got, out);
    }
    free(lit);
    delete sc;
    delete st;
    fclose(in);
    if (fclose(out)) return 2;
    return 0;
}
