// zstd_dec_host.cpp -- the decoder core (backuwup_amd/csrc/bw_zstd_dec_core.h) as a plain host
// program, built by tests/test_zstd_decode_host.py with -fsanitize=address,undefined: the same code
// the kernel runs, over frames that come off a disk and may be damaged.
//
//   zstd_dec_host IN OUT
// IN:  u32 n, then per case u32 src_len, u32 dst_cap, src bytes.
// OUT: per case i32 error (zd::Err), u32 out_len, u32 canary_ok, out bytes.
// Every frame is decoded from a heap copy of exactly src_len bytes (a read past it is an ASan
// report) into a buffer of dst_cap bytes followed by a 64-byte canary.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../backuwup_amd/csrc/bw_zstd_dec_core.h"

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
        uint8_t* src = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(src, 1, len, in) != len) return 2;
        uint8_t* dst = (uint8_t*)malloc((size_t)cap + 64);
        memset(dst, 0xEE, cap);
        memset(dst + cap, 0xA5, 64);
        size_t got = 0;
        zd::SerialExec x;
        const int32_t e = zd::decode_frame(src, len, dst, cap, st, sc, lit, &got, x);
        uint32_t canary = 1;
        for (int k = 0; k < 64; k++) canary &= dst[cap + k] == 0xA5;
        const uint32_t g = (uint32_t)got;
        fwrite(&e, 4, 1, out);
        fwrite(&g, 4, 1, out);
        fwrite(&canary, 4, 1, out);
        if (g) fwrite(dst, 1, g, out);
        free(dst);
        free(src);
    }
    free(lit);
    delete sc;
    delete st;
    fclose(in);
    if (fclose(out)) return 2;
    return 0;
}
