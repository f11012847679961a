// bw_find_host.h -- the pattern language of find (include/backuwup_gpu_pack.h, "find"): a glob over an
// item's path, compiled to a bit-parallel automaton of at most 64 states.  The state set of an item is one
// uint64_t per pattern; fd_step is the per-byte rule, and the one statement of it: k_fd_match
// (bw_find.hip) includes this header and runs the same arithmetic that tests/cpp/find_selftest.cpp traces
// on the host.  The compiler (fd_compile) is host code; the step, the accept test and the step over a
// '/' are host and device.  Free of HIP so that a plain C++ program can include it.  Off the chunk ->
// hash -> dedup path (backuwup_amd/build.py OFF_PATH).
//
// The path of an item is its names from the root's child down, joined by '/'; the automaton reads it
// as if every component, the last included, ended in '/'.  States, one bit each, in pattern order:
//   a literal byte, '?', a class   one state: the byte it accepts leads to the next state
//   '*'                            one state: stays on every byte but '/', and is passed over for free
//   the end of a component         one state: '/' leads to the next state
//   a '**' component               one state for the component and its '/': stays on every byte, and a
//                                  '/' read in it, or a '/' that enters it, also enters the next state
// A floating pattern has a '**' state in front.  Runs of '*' inside a component and runs of '**'
// components are one state each.  A pattern matches an item when a '/' after its name would reach the
// end of the pattern (acc); what a Dir hands to its children is the state after that '/'.  A state set
// of zero can never match again: nothing below such a Dir is looked at.
//   '?' and a negated class accept one code point byte by byte: an ASCII byte or a lead byte, and the
// state behind them stays in place over continuation bytes 0x80..0xBF (cont).  The names on the device
// are valid UTF-8 (the tree parser refuses others), so that is exact.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "bw_store_layout.h"

namespace bw {

constexpr uint32_t FD_MAX_STATES = 64;
constexpr uint32_t FD_MAX_PATTERNS = 32;

// What the step needs of a pattern beside its 256 byte masks.
struct FdPat {
    uint64_t star;   // the '*' states
    uint64_t dstar;  // the '**' states
    uint64_t cont;   // the states behind a '?' or a negated class
    uint64_t acc;    // the states from which a '/' reaches the end of the pattern
    uint64_t init;   // the states at the root's children
    uint64_t valid;  // the pattern's states: what a shift carries past the last of them is dropped
    uint32_t n_states, dir_only;
};

struct FdCompiled {
    FdPat p;
    uint64_t mask[256];  // mask[b]: the states whose byte b leads to the next state
};

// One byte of the path.  mask: the pattern's 256 byte masks, wherever they live, `stride` words apart
// (1 in FdCompiled; the kernel keeps the patterns' masks of one byte side by side in LDS).
BW_HOST_DEVICE static inline uint64_t fd_step(const uint64_t* mask, uint32_t stride, const FdPat& p, uint64_t s, uint8_t b) {
    const bool slash = b == '/', cont = (b & 0xC0) == 0x80;
    const uint64_t stay = s & (p.dstar | (slash ? 0 : p.star) | (cont ? p.cont : 0));
    uint64_t t = ((s & mask[(uint32_t)b * stride]) << 1) | stay;
    if (slash) t |= (t & p.dstar) << 1;  // a '/' in or into a '**': the next component may start here
    t |= (t & p.star) << 1;              // a '*' matches nothing as well
    return t & p.valid;
}

BW_HOST_DEVICE static inline bool fd_accepts(const FdPat& p, uint64_t s) { return (s & p.acc) != 0; }

// What a Dir hands down: the state at the start of its children's names.
BW_HOST_DEVICE static inline uint64_t fd_after_slash(const uint64_t* mask, uint32_t stride, const FdPat& p, uint64_t s) {
    return fd_step(mask, stride, p, s, '/');
}

// ------------------------------------------------------------------ the compiler (host)
static inline bool fd_utf8_ok(const uint8_t* p, uint64_t n) {
    for (uint64_t i = 0; i < n;) {
        const uint8_t b = p[i];
        uint32_t more, lo = 0x80, hi = 0xBF;
        if (b < 0x80) { i++; continue; }
        if (b >= 0xC2 && b <= 0xDF) more = 1;
        else if (b >= 0xE0 && b <= 0xEF) { more = 2; if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; }
        else if (b >= 0xF0 && b <= 0xF4) { more = 3; if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; }
        else return false;
        if (i + more >= n) return false;
        if (p[i + 1] < lo || p[i + 1] > hi) return false;
        for (uint32_t k = 2; k <= more; k++)
            if ((p[i + k] & 0xC0) != 0x80) return false;
        i += more + 1;
    }
    return true;
}

struct FdAtom {
    enum Type { SET, STAR, SLASH, DSTAR } type;
    bool wide;         // '?' or a negated class: a whole code point
    uint64_t set[4];   // SET: the bytes it accepts
};

static inline void fd_set_add(uint64_t* set, uint32_t b, bool icase) {
    set[b >> 6] |= 1ull << (b & 63);
    if (!icase) return;
    if (b >= 'a' && b <= 'z') b -= 32;
    else if (b >= 'A' && b <= 'Z') b += 32;
    set[b >> 6] |= 1ull << (b & 63);
}

// pat[0 .. len) -> out.  0, or -1 with `why`; out.p.n_states holds the states the pattern needs either
// way once it parsed (more than FD_MAX_STATES is the refusal "needs N states").
static inline int fd_compile(const uint8_t* pat, uint64_t len, bool icase, FdCompiled& out, std::string& why) {
    out = FdCompiled();
    if (!len) { why = "an empty pattern"; return -1; }
    if (!fd_utf8_ok(pat, len)) { why = "a pattern that is not valid UTF-8"; return -1; }
    std::vector<FdAtom> atoms, comp;
    uint64_t i = 0;
    if (pat[0] == '/') i = 1;
    else atoms.push_back(FdAtom{FdAtom::DSTAR, false, {0, 0, 0, 0}});
    bool dir_only = false;
    for (;;) {  // one component per turn
        comp.clear();
        const uint64_t start = i;
        bool plain_stars = true;  // nothing but unescaped '*' so far
        while (i < len && pat[i] != '/') {
            const uint8_t c = pat[i++];
            FdAtom a{FdAtom::SET, false, {0, 0, 0, 0}};
            if (c == '*') {
                if (comp.empty() || comp.back().type != FdAtom::STAR) comp.push_back(FdAtom{FdAtom::STAR, false, {0, 0, 0, 0}});
                continue;
            }
            plain_stars = false;
            if (c == '?') {
                a.wide = true;
                for (uint32_t b = 0; b < 256; b++)
                    if (b != '/' && (b < 0x80 || b >= 0xC0)) fd_set_add(a.set, b, false);
            } else if (c == '\\') {
                if (i == len) { why = "a dangling backslash"; return -1; }
                if (pat[i] == '/') { why = "an escaped '/'"; return -1; }
                fd_set_add(a.set, pat[i++], icase);
            } else if (c == '[') {
                bool neg = false;
                if (i < len && (pat[i] == '!' || pat[i] == '^')) { neg = true; i++; }
                uint64_t in[4] = {0, 0, 0, 0};
                bool first = true, closed = false;
                while (i < len) {
                    uint8_t lo = pat[i++];
                    if (lo == ']' && !first) { closed = true; break; }
                    first = false;
                    if (lo == '\\') {
                        if (i == len) { why = "a dangling backslash"; return -1; }
                        lo = pat[i++];
                    }
                    uint8_t hi = lo;
                    if (i + 1 < len && pat[i] == '-' && pat[i + 1] != ']') {
                        hi = pat[i + 1];
                        i += 2;
                        if (hi == '\\') {
                            if (i == len) { why = "a dangling backslash"; return -1; }
                            hi = pat[i++];
                        }
                    }
                    if (lo >= 0x80 || hi >= 0x80) { why = "a class member that is not ASCII"; return -1; }
                    if (lo == '/' || hi == '/') { why = "a '/' inside a class"; return -1; }
                    if (hi < lo) { why = "a class range that runs backwards"; return -1; }
                    for (uint32_t b = lo; b <= hi; b++)
                        if (b != '/') fd_set_add(in, b, icase);
                }
                if (!closed) { why = "an unterminated class"; return -1; }
                a.wide = neg;
                for (uint32_t b = 0; b < 256; b++) {
                    const bool member = (in[b >> 6] >> (b & 63)) & 1;
                    if (neg ? (!member && b != '/' && (b < 0x80 || b >= 0xC0)) : member) fd_set_add(a.set, b, false);
                }
            } else {
                fd_set_add(a.set, c, icase);
            }
            comp.push_back(a);
        }
        const bool last = i == len;
        if (i == start) {  // an empty component: only a trailing '/' may leave one
            if (!last || start <= 1) { why = "an empty component"; return -1; }
            dir_only = true;
            break;
        }
        if (plain_stars && i - start == 2) {  // the component is exactly "**"
            if (atoms.empty() || atoms.back().type != FdAtom::DSTAR) atoms.push_back(FdAtom{FdAtom::DSTAR, false, {0, 0, 0, 0}});
        } else {
            atoms.insert(atoms.end(), comp.begin(), comp.end());
            atoms.push_back(FdAtom{FdAtom::SLASH, false, {0, 0, 0, 0}});
        }
        if (last) break;
        i++;  // the '/'
    }
    FdPat& p = out.p;
    p.dir_only = dir_only;
    p.n_states = (uint32_t)(atoms.size() > 0xffffffffull ? 0xffffffffull : atoms.size());
    if (atoms.size() > FD_MAX_STATES) {
        why = "a pattern that needs " + std::to_string(atoms.size()) + " states (at most 64)";
        return -1;
    }
    const uint64_t n = atoms.size();
    for (uint64_t k = 0; k < n; k++) {
        const FdAtom& a = atoms[k];
        const uint64_t bit = 1ull << k;
        if (a.type == FdAtom::STAR) p.star |= bit;
        else if (a.type == FdAtom::DSTAR) p.dstar |= bit;
        else if (a.type == FdAtom::SLASH) out.mask['/'] |= bit;
        else {
            for (uint32_t b = 0; b < 256; b++)
                if ((a.set[b >> 6] >> (b & 63)) & 1) out.mask[b] |= bit;
            if (a.wide) p.cont |= bit << 1;  // a SET is never the last state
        }
    }
    // a '/' reaches the end from the last state, and through a closing '**' from the state before it
    p.acc = 1ull << (n - 1);
    if (atoms[n - 1].type == FdAtom::DSTAR && n >= 2) p.acc |= 1ull << (n - 2);
    p.valid = n == 64 ? ~0ull : (1ull << n) - 1;
    p.init = 1;
    p.init |= (p.init & p.dstar) << 1;
    p.init |= (p.init & p.star) << 1;
    p.init &= p.valid;
    return 0;
}

}  // namespace bw
