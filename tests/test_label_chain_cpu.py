"""CPU: the staging index arithmetic of csrc/label_chain.h (LcStager, shared by the Viterbi and CRF kernels), compiled for
the host into a stand-alone program with the address and undefined-behaviour sanitizers and run over every class ceiling,
class count, workgroup width and both a full and a one-entity last workgroup.

The program states the mapping on its own: element idx = k * 64 * EW + tid of the (C, 16, EW) slab is class c = idx / (16 EW),
step tt = idx % (16 EW) / EW, entity ew = idx % EW; it sits at (c * T + tt) * E + ew from input[b][0][t0][e0] and at
c * (16 EW + 1) + tt * EW + ew in a staging buffer. It then moves a chunk through fetch and commit on heap buffers of
exactly the sizes the kernels get, so a step outside them is the sanitizer's to report."""
import os
import subprocess

from tests.helpers import ROOT

PROGRAM = r'''
#include <cstdio>
#include <set>
#include <vector>
#include "label_chain.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 10) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

template <int CMAX>
static int run(int C, int EW, int rest) {
    constexpr int R = CMAX / 4;
    const int T = 37, e0 = 2 * EW, E = e0 + rest, row = 16 * EW + 1, limit = 35, t0 = 32;
    static_assert(LC_CHUNK == 16, "the test states the chunk itself");
    std::vector<int> seen((size_t)C * 16 * EW, 0);
    std::set<int> lds;
    std::vector<float> slab((size_t)C * T * E), stage((size_t)C * row, -2.0f);
    for (size_t i = 0; i < slab.size(); ++i) slab[i] = (float)(i + 1);
    int pairs = 0;
    for (int tid = 0; tid < 64 * EW; ++tid) {
        LcStager S;
        S.init(tid, C, T, E, EW, e0);
        for (int k = 0; k < R; ++k) {
            const int idx = k * 64 * EW + tid, c = idx / (16 * EW), tt = idx % (16 * EW) / EW, ew = idx % EW;
            const bool in_set = c < C && e0 + ew < E;
            CHECK(S.has(k) == in_set, "has: CMAX %d C %d EW %d rest %d tid %d k %d", CMAX, C, EW, rest, tid, k);
            if (!S.has(k) || !in_set) continue;
            ++pairs;
            ++seen[((size_t)c * 16 + tt) * EW + ew];
            CHECK(S.goff(k) == ((int64_t)c * T + tt) * E + ew, "goff: CMAX %d C %d EW %d tid %d k %d", CMAX, C, EW, tid, k);
            CHECK(S.soff(k) == c * row + tt * EW + ew, "soff: CMAX %d C %d EW %d tid %d k %d", CMAX, C, EW, tid, k);
            CHECK(S.soff(k) >= 0 && S.soff(k) < C * row, "soff range: CMAX %d C %d EW %d tid %d k %d", CMAX, C, EW, tid, k);
            lds.insert(S.soff(k));
        }
        float pre[R];
        S.fetch(slab.data() + e0, t0, limit, pre);
        S.commit(stage.data(), pre);
    }
    CHECK((int)lds.size() == pairs, "LDS offsets collide: CMAX %d C %d EW %d rest %d", CMAX, C, EW, rest);
    for (int c = 0; c < C; ++c)
        for (int tt = 0; tt < 16; ++tt)
            for (int ew = 0; ew < EW; ++ew) {
                const int n = seen[((size_t)c * 16 + tt) * EW + ew];
                CHECK(n == (e0 + ew < E ? 1 : 0), "covered %d times: CMAX %d C %d EW %d c %d tt %d ew %d", n, CMAX, C, EW, c, tt, ew);
                if (e0 + ew >= E) continue;
                const float want = t0 + tt < limit ? slab[((size_t)c * T + t0 + tt) * E + e0 + ew] : 0.0f;
                CHECK(stage[c * row + tt * EW + ew] == want, "staged value: CMAX %d C %d EW %d c %d tt %d ew %d", CMAX, C, EW, c, tt, ew);
            }
    return pairs;
}

int main() {
    long total = 0;
    int configs = 0;
    for (int EW = 1; EW <= 8; ++EW)
        for (int rest : {1, EW}) {
            for (int C : {1, 5, 8}) { total += run<8>(C, EW, rest); ++configs; }
            for (int C : {1, 9, 16}) { total += run<16>(C, EW, rest); ++configs; }
            for (int C : {1, 17, 32}) { total += run<32>(C, EW, rest); ++configs; }
            for (int C : {1, 33, 64}) { total += run<64>(C, EW, rest); ++configs; }
        }
    // the geometry and the dispatch, at both wave limits
    const LcGeometry g = lc_geometry(40, 5, 4), h = lc_geometry(6, 9, 8);
    CHECK(g.waves == 4 && g.groups == 2 && g.row == 65 && g.buf_floats == 40u * 65u, "geometry (40, 5, 4)");
    CHECK(h.waves == 8 && h.groups == 2 && h.row == 129 && h.buf_floats == 6u * 129u, "geometry (6, 9, 8)");
    for (int C = 1; C <= 64; ++C) {
        const int cmax = lc_dispatch_classes(C, [](auto c) { return (int)decltype(c)::value; });
        CHECK(cmax >= C && (cmax == 8 || cmax / 2 < C), "dispatch of %d classes: %d", C, cmax);
    }
    std::printf("configs %d pairs %ld failures %d\n", configs, total, failures);
    return failures ? 1 : 0;
}
'''


def test_the_stager_maps_threads_onto_the_slab_one_to_one(tmp_path):
    src, exe = tmp_path / 'label_chain_host.cpp', tmp_path / 'label_chain_host'
    src.write_text(PROGRAM)
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, '2g-gcn_amd', 'csrc'), str(src), '-o', str(exe)],
                   check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1].startswith('configs 192 pairs ') and run.stdout.strip().endswith('failures 0')
