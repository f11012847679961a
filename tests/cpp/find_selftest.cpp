// find_selftest.cpp -- the pattern compiler and the per-byte rule of find (backuwup_amd/csrc/bw_find_host.h) in
// a stand-alone program: state counts, refusals and step traces, printed for tests/test_find_host.py to
// compare with lines worked out by hand.  The kernel (k_fd_match, bw_find.hip) runs the same fd_step.
#include <cstdio>
#include <cstring>
#include <string>

#include "bw_find_host.h"

using namespace bw;

static void compile(const char* tag, const std::string& pat, bool icase = false) {
    FdCompiled fc;
    std::string why;
    if (fd_compile((const uint8_t*)pat.data(), pat.size(), icase, fc, why))
        std::printf("%s refused: %s\n", tag, why.c_str());
    else
        std::printf("%s states=%u init=%llx acc=%llx star=%llx dstar=%llx cont=%llx dir=%u\n", tag, fc.p.n_states,
                    (unsigned long long)fc.p.init, (unsigned long long)fc.p.acc, (unsigned long long)fc.p.star,
                    (unsigned long long)fc.p.dstar, (unsigned long long)fc.p.cont, fc.p.dir_only);
}

// the state after every byte of the path (its components joined by '/'), then the verdict and what a Dir hands down
static void trace(const char* tag, const std::string& pat, const std::string& path, bool icase = false) {
    FdCompiled fc;
    std::string why;
    if (fd_compile((const uint8_t*)pat.data(), pat.size(), icase, fc, why)) {
        std::printf("%s refused: %s\n", tag, why.c_str());
        return;
    }
    uint64_t s = fc.p.init;
    std::printf("%s", tag);
    for (unsigned char b : path) {
        s = fd_step(fc.mask, 1, fc.p, s, b);
        std::printf(" %llx", (unsigned long long)s);
    }
    std::printf(" match=%d down=%llx\n", (int)fd_accepts(fc.p, s), (unsigned long long)fd_after_slash(fc.mask, 1, fc.p, s));
}

int main() {
    compile("A jpg", "*.jpg");
    compile("A 64", "/" + std::string(63, 'a'));
    compile("A 65", "/" + std::string(64, 'a'));
    compile("A float64", std::string(62, 'a'));
    compile("A float65", std::string(63, 'a'));
    compile("A runs", "/a***b/**/**/c/");
    compile("A all", "**");
    compile("R empty", "");
    compile("R slash", "/");
    compile("R component", "a//b");
    compile("R class", "a[bc");
    compile("R backslash", "ab\\");
    compile("R utf8", "a\xc3");
    compile("R overlong", "\xc0\xaf");
    compile("R member", "[\xc3\xa9]");
    compile("R classslash", "[a/b]");
    compile("R escslash", "a\\/b");
    compile("R range", "[z-a]");
    trace("T two", "/a?", "a\xc3\xa9");
    trace("T three", "/a?", "a\xe2\x82\xac");
    trace("T four", "/a?", "a\xf0\x9f\x98\x80");
    trace("T twice", "/a?", "a\xc3\xa9\xc3\xa9");
    trace("T neg", "/[!a]b", "\xe2\x82\xac" "b");
    trace("T zero", "/a/**/b", "a/b");
    trace("T one", "/a/**/b", "a/x/b");
    trace("T mid", "/a/**/b", "a/xb");
    trace("T icase", "/Ab", "aB", true);
    trace("T case", "/Ab", "aB");
    trace("T float", "*.jpg", "x/y.jpg");
    trace("T last", "/" + std::string(63, 'a'), std::string(63, 'a'));
    trace("T tail", "/a/**", "a");
    return 0;
}
