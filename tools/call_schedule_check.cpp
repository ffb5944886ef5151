// call_schedule_check.cpp -- the dispatch table of the one-launch polar call (host_prep.cpp: build_call_schedule) on a Kuhn lattice, as a
// stand-alone host program: no device, no Python.  Meant for a sanitizer build of the host code,
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I tetsim_amd/csrc \
//       tools/call_schedule_check.cpp tetsim_amd/csrc/host_prep.cpp tetsim_amd/csrc/partitioner.cpp -o call_schedule_check && ./call_schedule_check 12 55
// and for a look at a table: per lag the period, the tail, the wrapped and the empty entries.  Exit status 0 = every table passed
// check_call_schedule, the plain table is [tiles | particle blocks], a lag of a whole substep fell back and said so.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_prep.h"

using namespace tetsim;

static int run(uint32_t n) {
    const uint32_t n1 = n + 1u;
    std::vector<float> verts(3ull * n1 * n1 * n1);
    for (uint32_t k = 0; k < n1; k++)
        for (uint32_t j = 0; j < n1; j++)
            for (uint32_t i = 0; i < n1; i++) {
                float* p = &verts[3ull * (i + n1 * (j + n1 * k))];
                p[0] = static_cast<float>(i) / n; p[1] = 0.5f + static_cast<float>(j) / n; p[2] = static_cast<float>(k) / n;
            }
    static const int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    std::vector<int32_t> tets;
    for (uint32_t k = 0; k < n; k++)
        for (uint32_t j = 0; j < n; j++)
            for (uint32_t i = 0; i < n; i++)
                for (const auto& perm : kPerm) {
                    uint32_t p[3] = {i, j, k};
                    tets.push_back(static_cast<int32_t>(p[0] + n1 * (p[1] + n1 * p[2])));
                    for (int a : perm) { p[a]++; tets.push_back(static_cast<int32_t>(p[0] + n1 * (p[1] + n1 * p[2]))); }
                }
    const uint32_t nv = n1 * n1 * n1, nt = static_cast<uint32_t>(tets.size() / 4);
    const std::vector<uint32_t> order = morton_vertex_order(verts.data(), nv, 0, nv);
    std::vector<int32_t> to_dev(nv);
    std::vector<float> lverts(3ull * nv);
    for (uint32_t i = 0; i < nv; i++) {
        to_dev[order[i]] = static_cast<int32_t>(i);
        for (int c = 0; c < 3; c++) lverts[3ull * i + c] = verts[3ull * order[i] + c];
    }
    for (auto& id : tets) id = to_dev[id];
    const Incidence inc = build_incidence(tets.data(), nt, nv, false, false);
    BlockPlan B;
    build_blocks(lverts.data(), tets.data(), nt, nv, nv, inc, &B);
    const uint32_t nb = B.num_blocks, npb = (nv + kBlockTile - 1u) / kBlockTile, plain = ((((nb + 7u) & ~7u) + npb) + 7u) & ~7u;
    std::printf("%u cells: %u tets, %u particles, %u tiles, %u particle blocks, plain period %u\n", n, nt, nv, nb, npb, plain);
    int bad = 0;
    const uint32_t lags[] = {0u, 1u, 2u, 3u, 4u, 8u, 16u, 32u, 64u, nb + 1u};
    for (uint32_t lag : lags) {
        CallSchedule S;
        build_call_schedule(B.blk_verts.data(), B.blk_vert_off.data(), nb, B.vp_ell.data(), B.vp_cols, B.nv_pad, nv, lag, &S);
        const std::string e = check_call_schedule(B.blk_verts.data(), B.blk_vert_off.data(), nb, B.vp_ell.data(), B.vp_cols, B.nv_pad, nv, S.entry.data(), S.period, S.tail);
        uint32_t wrapped = 0, empty = 0;
        for (uint32_t x : S.entry) { wrapped += (x >> 30) == kSchedParticles && (x & kSchedWrapped) ? 1u : 0u; empty += (x >> 30) == kSchedEmpty ? 1u : 0u; }
        std::printf("  lag %6u: period %6u  tail %5u  wrapped %4u  empty %5u  %s%s%s\n", lag, S.period, S.tail, wrapped, empty,
                    S.fell_back ? "FELL BACK: " : "", S.why.c_str(), e.empty() ? "" : ("  CHECK FAILED: " + e).c_str());
        if (!e.empty() || S.entry.size() != S.period) bad = 1;
        if (lag == 0 || S.fell_back) {   // the plain order, entry by entry
            if (S.period != plain || S.tail != 0) bad = 1;
            const uint32_t per_xcd = (nb + 7u) / 8u, tet_blocks = per_xcd * 8u;
            for (uint32_t p = 0; p < S.period && p < plain; p++) {
                const uint32_t want = p < tet_blocks ? ((p & 7u) * per_xcd + (p >> 3) < nb ? sched_entry(kSchedTile, p) : sched_entry(kSchedEmpty, 0))
                                                     : p - tet_blocks < npb ? sched_entry(kSchedParticles, p - tet_blocks) : sched_entry(kSchedEmpty, 0);
                if (S.entry[p] != want) bad = 1;
            }
        }
        if (lag == nb + 1u && (!S.fell_back || S.why.empty())) bad = 1;
        if (lag == 0 && S.fell_back) bad = 1;
    }
    return bad;
}

int main(int argc, char** argv) {
    int bad = 0;
    if (argc < 2) bad |= run(12);
    for (int i = 1; i < argc; i++) bad |= run(static_cast<uint32_t>(std::strtoul(argv[i], nullptr, 10)));
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
