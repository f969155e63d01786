"""The two column lists of the swept-segment queries (csrc/cd_columns.h: SweepSegmentCols, SweepSegmentRowCols), checked by the scheme of
tests/test_columns_layout.py: a stand-alone C++ program under the address and undefined-behaviour sanitizers -- no GPU, nothing
loaded into Python.

For each list the program restates the columns (name, element size, elements an item) and checks against a real malloc of exactly
bytes * cap, for caps 1, 2, 3, 7, 64, 65, that
  - the bytes an item equal a literal sum,
  - every column is aligned to its element type and lies inside the block,
  - the columns are pairwise disjoint and together cover the block exactly,
  - every element of every column can be written (the sanitizer is the bounds check)."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-computing-course_amd", "csrc")
CXX = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC]

PROGRAM = r"""
#include "cd_columns.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace cd;

struct Col { const char *name; char *p; uint64_t size, elems; };
static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("  [%s]\n", #cond); ++bad; } } while (0)
#define C(k, member, elems) Col{#member, reinterpret_cast<char *>(k.member), sizeof(*k.member), elems}

template <class Make> static void check(const char *what, uint64_t want_bytes, uint64_t got_bytes, Make make)
{
    CHECK(got_bytes == want_bytes, "%s: %llu bytes an item, not %llu", what, (unsigned long long)got_bytes, (unsigned long long)want_bytes);
    for (uint64_t cap : {1, 2, 3, 7, 64, 65}) {
        const uint64_t total = want_bytes * cap;
        char *block = static_cast<char *>(std::malloc(total));
        std::vector<Col> cols;
        make(block, cap, cols);
        uint64_t covered = 0;
        for (const Col &c : cols) {
            const uint64_t len = c.size * c.elems * cap;
            CHECK(reinterpret_cast<uintptr_t>(c.p) % c.size == 0, "%s cap %llu: %s is misaligned", what, (unsigned long long)cap, c.name);
            CHECK(c.p >= block && c.p + len <= block + total, "%s cap %llu: %s leaves the block", what, (unsigned long long)cap, c.name);
            covered += len;
        }
        CHECK(covered == total, "%s cap %llu: the columns hold %llu of %llu bytes", what, (unsigned long long)cap, (unsigned long long)covered, (unsigned long long)total);
        std::vector<Col> by = cols;
        std::sort(by.begin(), by.end(), [](const Col &a, const Col &b) { return a.p < b.p; });
        for (size_t i = 0; i + 1 < by.size(); ++i)
            CHECK(by[i].p + by[i].size * by[i].elems * cap <= by[i + 1].p, "%s cap %llu: %s overlaps %s", what, (unsigned long long)cap, by[i].name, by[i + 1].name);
        if (!bad)                               // (a list that is wrong is reported above, not by the sanitizer's abort)
            for (const Col &c : cols) std::memset(c.p, 0xa5, c.size * c.elems * cap);
        std::free(block);
    }
}

int main()
{
    // the item (13), toi, dist, s, on_seg, on_tri, uv: 24 doubles; face, ID: 2 words; feature, end, cross, side: 4 bytes
    check("swept segment", 24 * 8 + 2 * 4 + 4, column_bytes<SweepSegmentCols>(), [](char *b, uint64_t cap, std::vector<Col> &o) {
        const SweepSegmentCols k = carve<SweepSegmentCols>(b, cap);
        o = {C(k, items, 13), C(k, toi, 1), C(k, dist, 1), C(k, s, 1), C(k, on_seg, 3), C(k, on_tri, 3), C(k, uv, 2), C(k, face, 1), C(k, ids, 1),
             C(k, feature, 1), C(k, end, 1), C(k, cross, 1), C(k, side, 1)}; });
    // toi, s, on_seg, on_tri, uv: 10 doubles; ID: 1 word; feature, end, cross, side: 4 bytes
    check("swept segment rows", 10 * 8 + 4 + 4, column_bytes<SweepSegmentRowCols>(), [](char *b, uint64_t cap, std::vector<Col> &o) {
        const SweepSegmentRowCols k = carve<SweepSegmentRowCols>(b, cap);
        o = {C(k, toi, 1), C(k, s, 1), C(k, on_seg, 3), C(k, on_tri, 3), C(k, uv, 2), C(k, ids, 1), C(k, feature, 1), C(k, end, 1), C(k, cross, 1), C(k, side, 1)}; });
    std::printf("%d failed\n", bad);
    return bad != 0;
}
"""


def test_sweep_segment_column_lists_under_sanitizers(tmp_path):
    src = tmp_path / "sweep_segment_columns_layout.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "sweep_segment_columns_layout")
    cc = subprocess.run(CXX + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)                # (the sanitizers' runtime is linked into the program)
    assert run.returncode == 0 and run.stdout.strip().endswith("0 failed"), run.stdout + run.stderr
