"""The host arithmetic of the tree-chain fetch that the diff walk and the parent match share
(backuwup_amd/csrc/bw_walk_host.h) in a stand-alone C++ program: the take table of a sub-batch, the
segments it pushes and the totals it adds, from hand-written header lists, and the layout of a level's
segments after the stable sort.  Every expected value below is worked out by hand.  The fetch itself
runs in tests/test_gpu_diff_walk.py and tests/test_gpu_parent_match.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

HOST_CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "bw_walk_host.h"
using namespace bw;
static RsTreeHdr hdr(uint32_t status, uint32_t kind, uint64_t name_len, uint64_t n_children, uint32_t has_next) {
    RsTreeHdr h;
    memset(&h, 0, sizeof(h));
    h.status = status; h.kind = kind; h.name_len = name_len; h.n_children = n_children; h.has_next = has_next;
    return h;
}
static void say_take(const char* tag, const std::vector<WkTake>& take) {
    for (size_t k = 0; k < take.size(); k++)
        std::printf("%s take %zu ref=%u cst=%u stage=%llu rows=%llu name=%llu next=%lld seg=%lld\n", tag, k, take[k].ref,
                    take[k].cst, (unsigned long long)take[k].stage, (unsigned long long)take[k].n_rows,
                    (unsigned long long)take[k].name_off, (long long)take[k].next, (long long)take[k].seg);
}
static void say_add(const char* tag, const WkAdd& a) {
    std::printf("%s add rows=%llu names=%llu segs=%llu\n", tag, (unsigned long long)a.rows, (unsigned long long)a.names,
                (unsigned long long)a.segs);
}
static void say_segs(const char* tag, const std::vector<WkSeg>& segs) {
    for (const WkSeg& g : segs)
        std::printf("%s seg node=%u sid=%u stage=%llu count=%llu\n", tag, g.node, g.sid, (unsigned long long)g.stage,
                    (unsigned long long)g.count);
}
static void say_u32(const char* tag, const char* what, const std::vector<uint32_t>& v) {
    std::printf("%s %s", tag, what);
    for (uint32_t x : v) std::printf(" %u", x);
    std::printf("\n");
}
int main() {
    {   // A: one sub-batch of first pieces that give header, name, rows and next_sibling (the diff walk's round 0),
        // into a level that already holds 100 rows and 7 name bytes
        WkLevel L;
        L.stage_rows = 100; L.name_total = 7;
        const std::vector<uint32_t> ref = {0, 1, 2, 3, 4, 5, 6}, ref_owner = {0, 1, 2, 3, 4, 5, 6};
        const std::vector<uint8_t> cst = {5, 0, 0, 0, 0, 0, 0};
        const std::vector<RsTreeHdr> hd = {
            hdr(0, 1, 3, 9, 1),   // the chain refused it: whatever the header says counts for nothing
            hdr(8, 1, 2, 4, 1),   // the parser refused it
            hdr(0, 1, 5, 0, 0),   // header only
            hdr(0, 0, 0, 0, 1),   // no rows, but a next_sibling
            hdr(0, 1, 4, 6, 0),   // rows, no next_sibling
            hdr(0, 1, 3, 2, 1),   // the owner is skipped: its name, nothing else
            hdr(0, 1, 1, 3, 1)};  // rows and a next_sibling
        std::vector<WkOwner> owners(7);
        owners[5].skip = 1;
        std::vector<WkTake> take(7);
        std::vector<uint32_t> next_owner;
        say_add("A", wk_plan(L, ref.data(), ref_owner.data(), cst.data(), hd.data(), 7, true, true, owners.data(), take.data(), next_owner));
        say_take("A", take);
        say_segs("A", L.segs);
        say_u32("A", "next_owner", next_owner);
        for (size_t i = 0; i < owners.size(); i++)
            std::printf("A owner %zu rows=%llu dir=%u\n", i, (unsigned long long)owners[i].n_rows, owners[i].dir);
        std::printf("A level rows=%llu names=%llu\n", (unsigned long long)L.stage_rows, (unsigned long long)L.name_total);
    }
    {   // B: chains, rows only (the parent match's chain fetch), one blob per sub-batch: two pieces of owner 0
        // arrive in different sub-batches with owner 1's between them
        WkLevel L;
        std::vector<WkOwner> owners(2);
        std::vector<uint32_t> ref_owner = {0, 1}, next_owner;
        const uint8_t ok = 0;
        const RsTreeHdr round0[2] = {hdr(0, 1, 9, 2, 1), hdr(0, 1, 9, 3, 1)}, round1[2] = {hdr(0, 1, 9, 4, 0), hdr(0, 1, 9, 1, 0)};
        for (int round = 0; round < 2; round++) {
            next_owner.clear();
            for (uint32_t k = 0; k < 2; k++) {
                std::vector<WkTake> take(1);
                const WkAdd add = wk_plan(L, &k, ref_owner.data(), &ok, (round ? round1 : round0) + k, 1, false, true, owners.data(),
                                          take.data(), next_owner);
                say_add("B", add);
                say_take("B", take);
                L.stage_rows += add.rows;
                L.name_total += add.names;
            }
            ref_owner = next_owner;
        }
        say_u32("B", "next_owner", next_owner);
        say_segs("B fetched", L.segs);
        const size_t n = L.segs.size();
        std::vector<uint64_t> row0(n + 1), stage(n);
        std::vector<uint32_t> node(n), sid(n);
        std::printf("B rows %llu\n", (unsigned long long)wk_layout(L.segs, row0.data(), stage.data(), node.data(), sid.data()));
        say_segs("B sorted", L.segs);
        for (size_t k = 0; k < n; k++)
            std::printf("B table %zu row0=%llu stage=%llu node=%u sid=%u\n", k, (unsigned long long)row0[k],
                        (unsigned long long)stage[k], node[k], sid[k]);
        std::printf("B end %llu owners %llu %llu\n", (unsigned long long)row0[n], (unsigned long long)owners[0].n_rows,
                    (unsigned long long)owners[1].n_rows);
    }
    {   // C: first pieces read for header and name only, owners that are no chain's (the parent match's children)
        WkLevel L;
        L.name_total = 40;
        const std::vector<uint32_t> ref = {1, 0}, ref_owner = {7, 9};
        const std::vector<uint8_t> cst = {0, 0};
        const std::vector<RsTreeHdr> hd = {hdr(0, 1, 2, 5, 1), hdr(0, 0, 6, 0, 0)};
        std::vector<WkTake> take(2);
        std::vector<uint32_t> next_owner;
        say_add("C", wk_plan(L, ref.data(), ref_owner.data(), cst.data(), hd.data(), 2, true, false, nullptr, take.data(), next_owner));
        say_take("C", take);
        std::printf("C segs %zu next %zu\n", L.segs.size(), next_owner.size());
        std::vector<uint64_t> row0(1, 77);
        const uint64_t rows = wk_layout(L.segs, row0.data(), nullptr, nullptr, nullptr);
        std::printf("C rows %llu row0 %llu\n", (unsigned long long)rows, (unsigned long long)row0[0]);
    }
    return 0;
}
"""

WANT = """
A add rows=9 names=13 segs=2
A take 0 ref=0 cst=5 stage=100 rows=0 name=7 next=-1 seg=-1
A take 1 ref=1 cst=0 stage=100 rows=0 name=7 next=-1 seg=-1
A take 2 ref=2 cst=0 stage=100 rows=0 name=7 next=-1 seg=-1
A take 3 ref=3 cst=0 stage=100 rows=0 name=12 next=0 seg=-1
A take 4 ref=4 cst=0 stage=100 rows=6 name=12 next=-1 seg=0
A take 5 ref=5 cst=0 stage=106 rows=0 name=16 next=-1 seg=-1
A take 6 ref=6 cst=0 stage=106 rows=3 name=19 next=1 seg=1
A seg node=4 sid=0 stage=100 count=6
A seg node=6 sid=1 stage=106 count=3
A next_owner 3 6
A owner 0 rows=0 dir=0
A owner 1 rows=0 dir=0
A owner 2 rows=0 dir=1
A owner 3 rows=0 dir=0
A owner 4 rows=6 dir=1
A owner 5 rows=0 dir=1
A owner 6 rows=3 dir=1
A level rows=100 names=7
B add rows=2 names=0 segs=1
B take 0 ref=0 cst=0 stage=0 rows=2 name=0 next=0 seg=0
B add rows=3 names=0 segs=1
B take 0 ref=1 cst=0 stage=2 rows=3 name=0 next=1 seg=1
B add rows=4 names=0 segs=1
B take 0 ref=0 cst=0 stage=5 rows=4 name=0 next=-1 seg=2
B add rows=1 names=0 segs=1
B take 0 ref=1 cst=0 stage=9 rows=1 name=0 next=-1 seg=3
B next_owner
B fetched seg node=0 sid=0 stage=0 count=2
B fetched seg node=1 sid=1 stage=2 count=3
B fetched seg node=0 sid=2 stage=5 count=4
B fetched seg node=1 sid=3 stage=9 count=1
B rows 10
B sorted seg node=0 sid=0 stage=0 count=2
B sorted seg node=0 sid=2 stage=5 count=4
B sorted seg node=1 sid=1 stage=2 count=3
B sorted seg node=1 sid=3 stage=9 count=1
B table 0 row0=0 stage=0 node=0 sid=0
B table 1 row0=2 stage=5 node=0 sid=2
B table 2 row0=6 stage=2 node=1 sid=1
B table 3 row0=9 stage=9 node=1 sid=3
B end 10 owners 6 4
C add rows=0 names=8 segs=0
C take 0 ref=1 cst=0 stage=0 rows=0 name=40 next=-1 seg=-1
C take 1 ref=0 cst=0 stage=0 rows=0 name=42 next=-1 seg=-1
C segs 0 next 0
C rows 0 row0 0
""".strip().splitlines()


def run_host(tmp_path, extra=()):
    src = tmp_path / "walk_host.cpp"
    src.write_text(HOST_CPP)
    exe = tmp_path / ("walk_host" + ("_san" if extra else ""))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", *extra, "-I", os.path.join(ROOT, "backuwup_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=180)
    return [ln.rstrip() for ln in subprocess.check_output([str(exe)], timeout=60).decode().splitlines()]


def test_take_table_segments_totals_and_layout(tmp_path):
    assert run_host(tmp_path) == WANT


def test_the_same_program_under_the_address_and_undefined_sanitizers(tmp_path):
    assert run_host(tmp_path, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == WANT
