"""The host arithmetic of impact (backuwup_amd/csrc/bw_impact_host.h) in a stand-alone C++ program, plain
and under the address and undefined sanitizers: the check that a taint vector holds only the two public
bits, the bound on the edges a sub-batch's decoded bytes can name, and the edge list's layout by level with the order a
sweep takes the levels in.  Every expected value below is worked out by hand.  The walks themselves run
in tests/test_gpu_impact.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

HOST_CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "bw_impact_host.h"
using namespace bw;
int main() {
    {   // A: the taint check
        const std::vector<uint8_t> ok = {0, 1, 2, 3, 0}, bit4 = {0, 3, 4, 8}, high = {1, 2, 0x83};
        std::printf("A %lld %lld %lld %lld\n", (long long)im_taint_check(ok.data(), ok.size()), (long long)im_taint_check(bit4.data(), bit4.size()),
                    (long long)im_taint_check(high.data(), high.size()), (long long)im_taint_check(nullptr, 0));
    }
    {   // B: a sub-batch: the chain refused blob 0; 31 bytes name no hash, 32 one, 95 two, 320,061 bytes 10,001
        const std::vector<uint8_t> cst = {3, 0, 0, 0, 0};
        const std::vector<uint64_t> len = {3200, 31, 32, 95, 320061};
        std::printf("B %llu %llu\n", (unsigned long long)im_edge_bound(cst.data(), len.data(), 5),
                    (unsigned long long)im_edge_bound(cst.data(), len.data(), 0));
    }
    {   // C: four levels, the second appends nothing; a count that goes backwards is refused and changes nothing
        ImLevels L;
        std::printf("C empty levels=%llu edges=%llu sweep=%zu\n", (unsigned long long)L.n_levels(), (unsigned long long)L.n_edges(), L.sweep().size());
        const bool a = L.close(5), b = L.close(5), c = L.close(12), d = L.close(11), e = L.close(13);
        std::printf("C close %d %d %d %d %d levels=%llu edges=%llu\n", a, b, c, d, e, (unsigned long long)L.n_levels(), (unsigned long long)L.n_edges());
        for (const auto& r : L.sweep()) std::printf("C range %llu %llu\n", (unsigned long long)r.first, (unsigned long long)r.second);
    }
    return 0;
}
"""

WANT = """
A -1 2 2 -1
B 10004 0
C empty levels=0 edges=0 sweep=0
C close 1 1 1 0 1 levels=4 edges=13
C range 12 13
C range 5 12
C range 0 5
""".strip().splitlines()


def run_host(tmp_path, extra=()):
    src = tmp_path / "impact_host.cpp"
    src.write_text(HOST_CPP)
    exe = tmp_path / ("impact_host" + ("_san" if extra else ""))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", *extra, "-I", os.path.join(ROOT, "backuwup_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=180)
    return [ln.rstrip() for ln in subprocess.check_output([str(exe)], timeout=60).decode().splitlines()]


def test_taint_check_edge_bound_and_level_layout(tmp_path):
    assert run_host(tmp_path) == WANT


def test_the_same_program_under_the_address_and_undefined_sanitizers(tmp_path):
    assert run_host(tmp_path, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == WANT
