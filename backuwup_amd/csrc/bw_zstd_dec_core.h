// bw_zstd_dec_core.h -- a zstd frame decoder written from RFC 8878: the whole format a single
// magicless frame without a dictionary can hold (unpack.rs:65-67 reads such frames through
// zstd::bulk::Decompressor with include_magicbytes(false)).  Every function is __host__ __device__
// under hipcc and a plain function under g++: the kernel (bw_zstd_dec.hip) and a stand-alone host
// program (tests/cpp/zstd_dec_host.cpp, run under ASan/UBSan) execute the same code.
//
// One frame is decoded by one driver, zd::decode_frame.  The driver is serial; what can run wide
// (the four Huffman streams, every copy) goes through an execution policy X:
//   x.for_streams(n, f)   f(k) for stream k < n (host: a loop; device: lane k)
//   x.any(v)              v or-ed over the participants of for_streams
//   x.copy / x.fill / x.match   the byte moves (device: all lanes of the wave)
//   x.sync()              writes of for_streams visible to every participant
// On the device every lane of a wave runs the driver with the same inputs, so its control flow is
// uniform and the tables it builds are written with the same values by every lane.
//
// Refused (per-frame error, never a fault): a non-zero dictionary id; the checksum flag (the
// reference's Compressor sets include_checksum(false), pack.rs:58-64, so no packfile carries one);
// a reserved block type; anything after the last block.  Every read is bounded by its section,
// every table description is checked, every backward bitstream must carry its end mark and be
// consumed exactly, and no byte is written outside [dst, dst + cap).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ZD_FN __host__ __device__ inline
#else
#define ZD_FN inline
#endif

namespace zd {

enum Err : int {
    OK = 0,
    E_HEADER = 1,      // frame header: truncated, reserved bit, window over 2^31
    E_DICT = 2,        // non-zero dictionary id
    E_CHECKSUM = 3,    // content checksum flag
    E_BLOCK = 4,       // block header: truncated, reserved type, size over 128 KiB or past the frame
    E_TRAILING = 5,    // bytes after the last block
    E_LITERALS = 6,    // literals section header or sizes
    E_HUF_TABLE = 7,   // Huffman tree description
    E_HUF_STREAM = 8,  // Huffman stream: end mark, jump table, not consumed exactly
    E_SEQ_HEADER = 9,  // sequence count, modes byte, missing table
    E_FSE_TABLE = 10,  // FSE table description
    E_SEQ_STREAM = 11, // sequences bitstream: end mark, underflow, not consumed exactly
    E_LIT_OVERRUN = 12,// literal lengths exceed the block's literals
    E_OFFSET = 13,     // offset 0 or before the start of the output
    E_BLOCK_SIZE = 14, // a block regenerates more than 128 KiB
    E_DST = 15,        // the frame regenerates more than dst_cap
    E_CONTENT_SIZE = 16// Frame_Content_Size differs from the regenerated size
};

constexpr uint32_t BLOCK_MAX = 128u * 1024;
constexpr uint32_t LIT_SLACK = 32;  // bytes behind the literals buffer (never read as literals)
constexpr int HUF_MAX_LOG = 11;     // RFC 8878 4.2.1: Max_Number_of_Bits

struct FseEntry {
    uint16_t base;
    uint8_t sym, nb;
};

struct FseTable {
    uint32_t log;
    uint32_t valid;
};

// Everything a frame carries from block to block: the three sequence tables, the Huffman table and
// the repeat offsets.  About 9.3 KiB; in LDS on the device.
struct State {
    FseEntry ll[512], of[256], ml[512];
    uint16_t huf[1u << HUF_MAX_LOG];  // sym | nbits << 8
    FseTable t_ll, t_of, t_ml;
    uint32_t huf_log, huf_valid;
    uint32_t rep[3];
};

// scratch of the table builders (device: LDS next to State)
struct Scratch {
    int16_t counts[256];
    uint16_t next[256];
    uint8_t weights[256];
    FseEntry wt[64];  // the FSE table of Huffman weights (accuracy log <= 6)
};

#define ZD_LL_BITS                                                                                                     \
    { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 }
#define ZD_LL_BASE                                                                                                     \
    { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512,    \
      1024, 2048, 4096, 8192, 16384, 32768, 65536 }
#define ZD_ML_BITS                                                                                                     \
    { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2,  \
      2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 }
#define ZD_ML_BASE                                                                                                     \
    { 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,    \
      32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771,    \
      65539 }
#define ZD_LL_DEFAULT                                                                                                  \
    { 4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1 }
#define ZD_ML_DEFAULT                                                                                                  \
    { 1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,  \
      1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1 }
#define ZD_OF_DEFAULT                                                                                                  \
    { 1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1 }

ZD_FN uint32_t highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v != 0

// up to 8 little-endian bytes at p[at ..], zero where at + k >= len
ZD_FN uint64_t load_le(const uint8_t* p, size_t len, size_t at) {
    uint64_t v = 0;
    if (at + 8 <= len) {
        memcpy(&v, p + at, 8);
        return v;
    }
    for (size_t k = 0; at + k < len && k < 8; k++) v |= (uint64_t)p[at + k] << (8 * k);
    return v;
}

// A forward bit reader over a table description (RFC 8878 4.1.1), bounded by its section.
struct FwdBits {
    const uint8_t* p;
    size_t len;
    size_t at;  // bits consumed
    ZD_FN uint32_t peek(uint32_t n) const {  // n <= 32
        return (uint32_t)((load_le(p, len, at >> 3) >> (at & 7)) & ((1ull << n) - 1));
    }
};

// A bitstream read from its last byte down (RFC 8878 4.1): the final byte's highest set bit is the
// end mark.  pos = bits not yet read; reading below 0 is an error the caller sees in `bad`.
struct BackBits {
    const uint8_t* p;
    size_t len;
    int64_t pos;
    uint32_t bad;
    ZD_FN bool init(const uint8_t* s, size_t n) {
        p = s;
        len = n;
        bad = 0;
        pos = 0;
        if (n == 0 || s[n - 1] == 0) return false;
        pos = (int64_t)(8 * n) - (int64_t)(8 - highbit(s[n - 1]));
        return true;
    }
    // the next n bits (n <= 32) without consuming; bits below the start read as zero
    ZD_FN uint32_t peek(uint32_t n) const {
        if (n == 0) return 0;
        const int64_t lo = pos - (int64_t)n;
        if (lo >= 0) return (uint32_t)((load_le(p, len, (size_t)(lo >> 3)) >> (lo & 7)) & ((1ull << n) - 1));
        if (pos <= 0) return 0;
        const uint64_t have = load_le(p, len, 0) & ((1ull << pos) - 1);  // pos < n <= 32
        return (uint32_t)(have << (uint32_t)(-lo));
    }
    ZD_FN void skip(uint32_t n) {
        pos -= (int64_t)n;
        if (pos < 0) bad = 1;
    }
    ZD_FN uint32_t read(uint32_t n) {
        const uint32_t v = peek(n);
        skip(n);
        return v;
    }
};

// ------------------------------------------------------------------ FSE tables (RFC 8878 4.1.1)

// The normalized counts of a table description at p[0 .. len) -> counts[0 .. *n_sym), the accuracy
// log and the bytes consumed.  max_sym / max_log: the limits of the table's use.
ZD_FN int read_ncount(const uint8_t* p, size_t len, uint32_t max_sym, uint32_t max_log, int16_t* counts,
                      uint32_t* n_sym, uint32_t* log_out, size_t* used) {
    if (len == 0) return E_FSE_TABLE;
    FwdBits b{p, len, 0};
    const uint32_t log = b.peek(4) + 5;
    b.at = 4;
    if (log > max_log) return E_FSE_TABLE;
    int32_t remaining = 1 << log;
    uint32_t n = 0;
    while (remaining > 0 && n <= max_sym) {
        if (b.at > 8 * len) return E_FSE_TABLE;
        const uint32_t bits = highbit((uint32_t)remaining + 1) + 1;
        uint32_t val = b.peek(bits);
        const uint32_t low = (1u << (bits - 1)) - 1;
        const uint32_t threshold = (1u << bits) - 1 - ((uint32_t)remaining + 1);
        if ((val & low) < threshold) {
            val &= low;
            b.at += bits - 1;
        } else {
            if (val > low) val -= threshold;
            b.at += bits;
        }
        const int32_t prob = (int32_t)val - 1;
        remaining -= prob < 0 ? -prob : prob;
        counts[n++] = (int16_t)prob;
        if (prob == 0) {
            for (;;) {
                if (b.at > 8 * len) return E_FSE_TABLE;
                const uint32_t rep = b.peek(2);
                b.at += 2;
                for (uint32_t k = 0; k < rep; k++) {
                    if (n > max_sym) return E_FSE_TABLE;
                    counts[n++] = 0;
                }
                if (rep != 3) break;
            }
        }
    }
    if (remaining != 0 || n > max_sym + 1 || b.at > 8 * len) return E_FSE_TABLE;
    *n_sym = n;
    *log_out = log;
    *used = (b.at + 7) >> 3;
    return OK;
}

// The decoding table of `counts` (sum of |counts| = 1 << log, checked by read_ncount or fixed).
ZD_FN int build_fse(FseEntry* t, uint32_t log, const int16_t* counts, uint32_t n_sym, uint16_t* next) {
    const uint32_t size = 1u << log;
    uint32_t high = size;
    for (uint32_t s = 0; s < n_sym; s++) {
        if (counts[s] == -1) {
            t[--high].sym = (uint8_t)s;
            next[s] = 1;
        } else {
            next[s] = (uint16_t)counts[s];
        }
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < n_sym; s++)
        for (int32_t k = 0; k < counts[s]; k++) {
            t[pos].sym = (uint8_t)s;
            do pos = (pos + step) & mask;
            while (pos >= high);
        }
    if (pos != 0) return E_FSE_TABLE;
    for (uint32_t i = 0; i < size; i++) {
        const uint32_t s = t[i].sym, n = next[s]++;
        const uint32_t nb = log - highbit(n);
        t[i].nb = (uint8_t)nb;
        t[i].base = (uint16_t)((n << nb) - size);
    }
    return OK;
}

// ------------------------------------------------------------------ Huffman (RFC 8878 4.2)

// The tree description at p[0 .. len) -> the decoding table in st; *used = its size in bytes.
ZD_FN int build_huffman(State* st, Scratch* sc, const uint8_t* p, size_t len, size_t* used) {
    if (len == 0) return E_HUF_TABLE;
    const uint32_t h = p[0];
    uint8_t* w = sc->weights;
    uint32_t n = 0;
    if (h >= 128) {  // direct: 4 bits per weight
        n = h - 127;
        const uint32_t nbytes = (n + 1) / 2;
        if (1 + (size_t)nbytes > len) return E_HUF_TABLE;
        for (uint32_t i = 0; i < n; i++) w[i] = (i & 1) ? (p[1 + i / 2] & 15) : (p[1 + i / 2] >> 4);
        *used = 1 + nbytes;
    } else {  // FSE-coded weights, two interleaved states
        if (h == 0 || 1 + (size_t)h > len) return E_HUF_TABLE;
        uint32_t n_sym, log;
        size_t hdr;
        if (read_ncount(p + 1, h, 255, 6, sc->counts, &n_sym, &log, &hdr)) return E_HUF_TABLE;
        if (build_fse(sc->wt, log, sc->counts, n_sym, sc->next)) return E_HUF_TABLE;
        BackBits b;
        if (!b.init(p + 1 + hdr, h - hdr)) return E_HUF_TABLE;
        uint32_t s1 = b.read(log), s2 = b.read(log);
        if (b.bad) return E_HUF_TABLE;
        for (;;) {  // the stream ends when a state update runs out of bits
            if (n > 253) return E_HUF_TABLE;
            w[n++] = sc->wt[s1].sym;
            if (b.pos < (int64_t)sc->wt[s1].nb) {
                w[n++] = sc->wt[s2].sym;
                break;
            }
            s1 = sc->wt[s1].base + b.read(sc->wt[s1].nb);
            w[n++] = sc->wt[s2].sym;
            if (b.pos < (int64_t)sc->wt[s2].nb) {
                w[n++] = sc->wt[s1].sym;
                break;
            }
            s2 = sc->wt[s2].base + b.read(sc->wt[s2].nb);
        }
        *used = 1 + h;
    }
    // the last weight completes the next power of two
    uint32_t total = 0, rank[HUF_MAX_LOG + 2] = {};
    for (uint32_t i = 0; i < n; i++) {
        if (w[i] > HUF_MAX_LOG) return E_HUF_TABLE;
        if (w[i]) total += 1u << (w[i] - 1);
    }
    if (total == 0) return E_HUF_TABLE;
    const uint32_t log = highbit(total) + 1;
    if (log > (uint32_t)HUF_MAX_LOG) return E_HUF_TABLE;
    const uint32_t rest = (1u << log) - total;
    if (rest & (rest - 1)) return E_HUF_TABLE;
    w[n++] = (uint8_t)(highbit(rest) + 1);
    for (uint32_t i = 0; i < n; i++) rank[w[i]]++;
    if (rank[1] < 2 || (rank[1] & 1)) return E_HUF_TABLE;  // a complete tree has an even number of deepest leaves
    // table positions by weight, symbols in order inside a weight
    uint32_t start[HUF_MAX_LOG + 2], at = 0;
    for (uint32_t r = 1; r <= log; r++) {
        start[r] = at;
        at += rank[r] << (r - 1);
    }
    if (at != (1u << log)) return E_HUF_TABLE;
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t r = w[s];
        if (!r) continue;
        const uint32_t span = 1u << (r - 1);
        const uint16_t e = (uint16_t)(s | ((log + 1 - r) << 8));
        for (uint32_t k = 0; k < span; k++) st->huf[start[r] + k] = e;
        start[r] += span;
    }
    st->huf_log = log;
    st->huf_valid = 1;
    return OK;
}

// One Huffman stream s[0 .. len) -> exactly n symbols at out.
ZD_FN int huf_stream(const State* st, const uint8_t* s, size_t len, uint8_t* out, uint32_t n) {
    BackBits b;
    if (!b.init(s, len)) return E_HUF_STREAM;
    const uint32_t log = st->huf_log;
    for (uint32_t i = 0; i < n; i++) {
        const uint16_t e = st->huf[b.peek(log)];
        b.skip(e >> 8);
        out[i] = (uint8_t)e;
    }
    return (b.bad || b.pos != 0) ? E_HUF_STREAM : OK;
}

// ------------------------------------------------------------------ sections

struct Literals {
    const uint8_t* ptr;  // raw: into the frame; Huffman: the literals buffer
    uint32_t size;
    uint32_t rle;  // 1: `size` copies of byte
    uint8_t byte;
};

// The literals section (RFC 8878 3.1.1.3.1) of a block body p[0 .. len): *used = its size.
template <class X>
ZD_FN int decode_literals(State* st, Scratch* sc, const uint8_t* p, size_t len, uint8_t* litbuf, Literals* L,
                          size_t* used, X& x) {
    if (len < 3) return E_LITERALS;  // the smallest block body: literals header, sequence count, one more byte
    const uint32_t kind = p[0] & 3, sf = (p[0] >> 2) & 3;
    L->rle = 0;
    L->byte = 0;
    if (kind < 2) {
        const uint32_t width = (sf & 1) == 0 ? 1 : (sf == 1 ? 2 : 3);
        const uint32_t v = p[0] | (width > 1 ? (uint32_t)p[1] << 8 : 0) | (width > 2 ? (uint32_t)p[2] << 16 : 0);
        const uint32_t regen = v >> (width == 1 ? 3 : 4);
        if (regen > BLOCK_MAX) return E_LITERALS;
        L->size = regen;
        if (kind == 0) {
            if ((size_t)width + regen > len) return E_LITERALS;
            L->ptr = p + width;
            *used = width + regen;
        } else {
            if ((size_t)width + 1 > len) return E_LITERALS;
            L->ptr = nullptr;
            L->rle = 1;
            L->byte = p[width];
            *used = width + 1;
        }
        return OK;
    }
    if (len < 5) return E_LITERALS;
    const uint32_t width = sf < 2 ? 3 : sf + 2, nbits = sf < 2 ? 10 : (sf == 2 ? 14 : 18);
    const uint64_t v = load_le(p, len, 0) >> 4;
    const uint32_t regen = (uint32_t)(v & ((1u << nbits) - 1));
    const uint32_t comp = (uint32_t)((v >> nbits) & ((1u << nbits) - 1));
    const uint32_t streams = sf == 0 ? 1 : 4;
    if (regen > BLOCK_MAX || (size_t)width + comp > len) return E_LITERALS;
    if (regen == 0) return E_LITERALS;  // Huffman-coded literals of size 0 code nothing (libzstd refuses them with 4 streams, 1.4.8 not with 1)
    const uint8_t* s = p + width;
    size_t left = comp;
    if (kind == 2) {
        size_t t;
        if (int e = build_huffman(st, sc, s, left, &t)) return e;
        s += t;
        left -= t;
    } else if (!st->huf_valid) {
        return E_LITERALS;  // treeless literals with no earlier tree
    }
    x.sync();  // the table is complete before any participant decodes with it
    if (left == 0) return E_HUF_STREAM;
    const uint8_t* sp[4];
    uint32_t sl[4], so[4], sn[4];
    if (streams == 1) {
        sp[0] = s;
        sl[0] = (uint32_t)left;
        so[0] = 0;
        sn[0] = regen;
    } else {
        if (left < 10 || regen == 0) return E_HUF_STREAM;  // jump table + one byte per stream
        const uint32_t seg = (regen + 3) / 4;
        if (3 * seg > regen) return E_HUF_STREAM;  // RFC 8878 4.2.2: the last stream holds the remainder
        uint32_t sum = 0;
        for (int k = 0; k < 3; k++) {
            sl[k] = s[2 * k] | ((uint32_t)s[2 * k + 1] << 8);
            sum += sl[k];
        }
        if ((size_t)sum + 6 >= left) return E_HUF_STREAM;
        sl[3] = (uint32_t)(left - 6 - sum);
        const uint8_t* q = s + 6;
        for (int k = 0; k < 4; k++) {
            sp[k] = q;
            q += sl[k];
            so[k] = (uint32_t)k * seg;
            sn[k] = k < 3 ? seg : regen - 3 * seg;
        }
    }
    int bad = 0;
    x.for_streams(streams, [&](uint32_t k) { bad |= huf_stream(st, sp[k], sl[k], litbuf + so[k], sn[k]); });
    bad = x.any(bad);
    x.sync();
    if (bad) return E_HUF_STREAM;
    L->ptr = litbuf;
    L->size = regen;
    *used = width + comp;
    return OK;
}

// One sequence table per its mode (RFC 8878 3.1.1.3.2.1); p advances over what the mode reads.
ZD_FN int seq_table(uint32_t mode, FseEntry* t, FseTable* info, Scratch* sc, const uint8_t*& p, const uint8_t* end,
                    uint32_t max_sym, uint32_t max_log, const int16_t* def_counts, uint32_t def_n, uint32_t def_log) {
    if (mode == 0) {
        for (uint32_t i = 0; i < def_n; i++) sc->counts[i] = def_counts[i];
        if (build_fse(t, def_log, sc->counts, def_n, sc->next)) return E_FSE_TABLE;
        info->log = def_log;
    } else if (mode == 1) {
        if (p >= end || *p > max_sym) return E_FSE_TABLE;
        t[0].sym = *p++;
        t[0].nb = 0;
        t[0].base = 0;
        info->log = 0;
    } else if (mode == 2) {
        uint32_t n_sym, log;
        size_t used;
        if (read_ncount(p, (size_t)(end - p), max_sym, max_log, sc->counts, &n_sym, &log, &used)) return E_FSE_TABLE;
        if (build_fse(t, log, sc->counts, n_sym, sc->next)) return E_FSE_TABLE;
        p += used;
        info->log = log;
    } else {
        return info->valid ? OK : E_SEQ_HEADER;  // repeat mode with no earlier table
    }
    return OK;
}

// A compressed block's body p[0 .. len) regenerated at dst + *op (block_start = *op on entry).
template <class X>
ZD_FN int decode_block(State* st, Scratch* sc, const uint8_t* p, size_t len, uint8_t* dst, size_t cap, size_t* op,
                       uint8_t* litbuf, X& x) {
    Literals L;
    size_t used;
    if (int e = decode_literals(st, sc, p, len, litbuf, &L, &used, x)) return e;
    const uint8_t* q = p + used;
    const uint8_t* const end = p + len;
    // sequences section header
    if (q >= end) return E_SEQ_HEADER;
    uint32_t nseq = *q++;
    if (nseq >= 128) {
        if (nseq == 255) {
            if (q + 2 > end) return E_SEQ_HEADER;
            nseq = q[0] + ((uint32_t)q[1] << 8) + 0x7F00;
            q += 2;
        } else {
            if (q + 1 > end) return E_SEQ_HEADER;
            nseq = ((nseq - 128) << 8) + *q++;
            if (nseq == 0) return E_SEQ_HEADER;  // RFC 8878 3.1.1.3.2.1: zero sequences is the single byte 0
        }
    }
    const size_t block_start = *op;
    const size_t limit = (cap - block_start) < BLOCK_MAX ? cap : block_start + BLOCK_MAX;  // this block's last + 1
    const bool cap_bound = limit == cap;
    size_t o = block_start;
    uint32_t lit_at = 0;
    if (nseq) {
        if (q >= end) return E_SEQ_HEADER;
        const uint32_t modes = *q++;
        if (modes & 3) return E_SEQ_HEADER;  // RFC 8878 3.1.1.3.2.1: Reserved bits
        const int16_t ll_def[] = ZD_LL_DEFAULT, ml_def[] = ZD_ML_DEFAULT, of_def[] = ZD_OF_DEFAULT;
        static_assert(sizeof(ll_def) == 36 * 2 && sizeof(ml_def) == 53 * 2 && sizeof(of_def) == 29 * 2, "default tables");
        if (int e = seq_table(modes >> 6, st->ll, &st->t_ll, sc, q, end, 35, 9, ll_def, 36, 6)) return e;
        if (int e = seq_table((modes >> 4) & 3, st->of, &st->t_of, sc, q, end, 31, 8, of_def, 29, 5)) return e;
        if (int e = seq_table((modes >> 2) & 3, st->ml, &st->t_ml, sc, q, end, 52, 9, ml_def, 53, 6)) return e;
        st->t_ll.valid = st->t_of.valid = st->t_ml.valid = 1;
        BackBits b;
        if (!b.init(q, (size_t)(end - q))) return E_SEQ_STREAM;
        const uint8_t ll_bits[] = ZD_LL_BITS, ml_bits[] = ZD_ML_BITS;
        const uint32_t ll_base[] = ZD_LL_BASE, ml_base[] = ZD_ML_BASE;
        static_assert(sizeof(ll_bits) == 36 && sizeof(ml_bits) == 53 && sizeof(ll_base) == 36 * 4 && sizeof(ml_base) == 53 * 4,
                      "code tables");
        uint32_t s_ll = b.read(st->t_ll.log), s_of = b.read(st->t_of.log), s_ml = b.read(st->t_ml.log);
        if (b.bad) return E_SEQ_STREAM;
        for (uint32_t i = 0; i < nseq; i++) {
            const FseEntry el = st->ll[s_ll], eo = st->of[s_of], em = st->ml[s_ml];
            // offset, match length, literal length, then the LL, ML, OF state updates
            const uint32_t oc = eo.sym;  // <= 31 by the table's symbol range
            const uint64_t ov = (1ull << oc) + b.read(oc);
            const uint32_t ml = ml_base[em.sym] + b.read(ml_bits[em.sym]);
            const uint32_t ll = ll_base[el.sym] + b.read(ll_bits[el.sym]);
            if (i + 1 < nseq) {
                s_ll = el.base + b.read(el.nb);
                s_ml = em.base + b.read(em.nb);
                s_of = eo.base + b.read(eo.nb);
            }
            if (b.bad) return E_SEQ_STREAM;
            // repeat offsets (RFC 8878 3.1.1.5)
            uint64_t off;
            if (ov > 3) {
                off = ov - 3;
                st->rep[2] = st->rep[1];
                st->rep[1] = st->rep[0];
                st->rep[0] = (uint32_t)(off > 0xffffffffull ? 0xffffffffu : off);
            } else {
                const uint32_t idx = (uint32_t)ov - 1 + (ll == 0);  // 0..3; 3 = rep1 - 1
                if (idx == 0) {
                    off = st->rep[0];
                } else {
                    off = idx == 3 ? (uint64_t)st->rep[0] - 1 : st->rep[idx];
                    if (off == 0 || off > 0xffffffffull) return E_OFFSET;
                    if (idx != 1) st->rep[2] = st->rep[1];
                    st->rep[1] = st->rep[0];
                    st->rep[0] = (uint32_t)off;
                }
            }
            if (ll > L.size - lit_at) return E_LIT_OVERRUN;
            if ((uint64_t)ll + ml > limit - o) return cap_bound ? E_DST : E_BLOCK_SIZE;
            if (off == 0 || off > o + ll) return E_OFFSET;
            if (ll) {
                if (L.rle) x.fill(dst + o, L.byte, ll);
                else x.copy(dst + o, L.ptr + lit_at, ll);
                lit_at += ll;
                o += ll;
            }
            x.match(dst + o, (size_t)off, ml);
            o += ml;
        }
        if (b.pos != 0) return E_SEQ_STREAM;
    } else if (q != end) {
        return E_SEQ_HEADER;  // bytes after an empty sequences section
    }
    const uint32_t rest = L.size - lit_at;
    if (rest > limit - o) return cap_bound ? E_DST : E_BLOCK_SIZE;
    if (rest) {
        if (L.rle) x.fill(dst + o, L.byte, rest);
        else x.copy(dst + o, L.ptr + lit_at, rest);
        o += rest;
    }
    *op = o;
    return OK;
}

// One magicless frame src[0 .. len) -> dst[0 .. *out_len), *out_len <= cap.  litbuf: BLOCK_MAX +
// LIT_SLACK bytes of scratch.  On an error *out_len is 0 and dst[0 .. cap) holds garbage.
template <class X>
ZD_FN int decode_frame(const uint8_t* src, size_t len, uint8_t* dst, size_t cap, State* st, Scratch* sc,
                       uint8_t* litbuf, size_t* out_len, X& x) {
    *out_len = 0;
    // no bytes: no frame.  ZSTD_decompressDCtx returns 0 there, so the reference's
    // Decompressor::decompress (unpack.rs:67) yields an empty blob, not an error.
    if (len == 0) return OK;
    // frame header (RFC 8878 3.1.1.1)
    const uint32_t fhd = src[0];
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did_flag = fhd & 3;
    if (fhd & 8) return E_HEADER;      // reserved bit
    if (fhd & 4) return E_CHECKSUM;
    size_t at = 1;
    if (!single) {
        if (at >= len) return E_HEADER;
        if ((src[at] >> 3) + 10u > 31u) return E_HEADER;
        at++;
    }
    const uint32_t did_bytes = did_flag == 3 ? 4 : did_flag;
    if (at + did_bytes > len) return E_HEADER;
    for (uint32_t k = 0; k < did_bytes; k++)
        if (src[at + k]) return E_DICT;
    at += did_bytes;
    const uint32_t fcs_bytes = fcs_flag == 0 ? single : (1u << fcs_flag);
    if (at + fcs_bytes > len) return E_HEADER;
    uint64_t fcs = 0;
    for (uint32_t k = 0; k < fcs_bytes; k++) fcs |= (uint64_t)src[at + k] << (8 * k);
    if (fcs_bytes == 2) fcs += 256;
    at += fcs_bytes;

    st->t_ll.valid = st->t_of.valid = st->t_ml.valid = 0;
    st->huf_valid = 0;
    st->rep[0] = 1;
    st->rep[1] = 4;
    st->rep[2] = 8;
    size_t op = 0;
    for (;;) {
        if (at + 3 > len) return E_BLOCK;
        const uint32_t h = src[at] | ((uint32_t)src[at + 1] << 8) | ((uint32_t)src[at + 2] << 16);
        at += 3;
        const uint32_t last = h & 1, type = (h >> 1) & 3, size = h >> 3;
        if (type == 3 || size > BLOCK_MAX) return E_BLOCK;
        if (type == 0) {
            if (size > len - at) return E_BLOCK;
            if (size > cap - op) return E_DST;
            if (size) x.copy(dst + op, src + at, size);
            at += size;
            op += size;
        } else if (type == 1) {
            if (at >= len) return E_BLOCK;
            if (size > cap - op) return E_DST;
            if (size) x.fill(dst + op, src[at], size);
            at += 1;
            op += size;
        } else {
            if (size > len - at || size >= BLOCK_MAX) return E_BLOCK;
            if (int e = decode_block(st, sc, src + at, size, dst, cap, &op, litbuf, x)) return e;
            at += size;
        }
        if (last) break;
    }
    if (at != len) return E_TRAILING;
    if (fcs_bytes && fcs != op) return E_CONTENT_SIZE;
    *out_len = op;
    return OK;
}

// Which matches must wait for the stores of a wide execution policy (the kernel's WaveExec; on the
// host the checking policy of tests/cpp/zstd_dec_hazard.cpp, which holds the rule to what was
// really stored).  The output grows upwards, so everything stored since the last barrier lies at or
// above the first address stored since then.
struct Hazard {
    const uint8_t* dirty;  // lowest output address stored since the last barrier (null: none)
    ZD_FN void synced() { dirty = nullptr; }
    ZD_FN void wrote(const uint8_t* d) {
        if (!dirty) dirty = d;
    }
    // a match of n bytes at d from d - off: does its source reach what was stored since the barrier?
    ZD_FN bool must_wait(const uint8_t* d, size_t off, uint32_t n) const {
        const uint8_t* s = d - off;
        const size_t span = off < n ? off : n;  // source bytes that exist before this match
        return dirty && s + span > dirty;
    }
};

// The serial execution policy (host programs; also a device thread working alone).
struct SerialExec {
    template <class F>
    ZD_FN void for_streams(uint32_t n, F f) {
        for (uint32_t k = 0; k < n; k++) f(k);
    }
    ZD_FN int any(int v) { return v; }
    ZD_FN void sync() {}
    ZD_FN void copy(uint8_t* d, const uint8_t* s, uint32_t n) { memcpy(d, s, n); }
    ZD_FN void fill(uint8_t* d, uint8_t b, uint32_t n) { memset(d, b, n); }
    ZD_FN void match(uint8_t* d, size_t off, uint32_t n) {
        const uint8_t* s = d - off;
        for (uint32_t i = 0; i < n; i++) d[i] = s[i];
    }
};

}  // namespace zd
