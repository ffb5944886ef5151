// query_closest.hip -- closest-point queries through the refitted tree of query_bvh.hip (include/tetsim.h: tetsim_closest_visual_device;
// query_device.h: the layout, and the refit this kernel runs behind; query_tree.h: the walk, and why tree shape and visit order cannot
// change a bit of the answer).  The answer is DEFINED without the tree (tests/closest_ref.py is the definition in numpy: brute force,
// three.js r160's Triangle.closestPointToPoint per triangle, one box predicate).  This walk's predicate:
//   * the bound lb of a box: a box that contains a triangle's box has lb <= the triangle's lb;
//   * a node is refused only if lb > max_distance^2, or a best exists and lb > its d2 (lb == best is entered: a lower triangle index
//     may tie);
//   * a triangle is tested against the box of its OWN corners, then by tri_closest.
// f64, every operation rounded separately: build with -ffp-contract=off.  One lane per query.
#include "dev_common.h"
#include "query_device.h"
#include "query_rays.h"
#include "query_tree.h"

#include <algorithm>
#include <cmath>

namespace tetsim {
namespace {

static_assert(sizeof(PointQueryIn) == 32 && sizeof(ClosestOut) == 64, "the records of include/tetsim.h");

// include/tetsim.h, "box bound": the squared distance from p to the box padded by e, never above the squared distance to anything inside
__device__ inline double box_bound(const double p[3], double e, const float lo[3], const float hi[3]) {
    double g[3];
    for (int k = 0; k < 3; k++) {
        const double L = static_cast<double>(lo[k]) - e, H = static_cast<double>(hi[k]) + e;
        const double g1 = L - p[k], g2 = p[k] - H;
        const double m = g1 > g2 ? g1 : g2;
        g[k] = m > 0.0 ? m : 0.0;
    }
    return g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
}

// three.js r160 Triangle.closestPointToPoint (Ericson, Real-Time Collision Detection 5.1.5), in the order of its operations; returns the
// region (include/tetsim.h: 1, 2, 3 the vertices a, b, c; 4, 5, 6 the edges ab, ac, bc; 0 the face), q and (v, w) with q = a + v ab + w ac
__device__ inline int tri_closest(const double p[3], const float4 A, const float4 B, const float4 C, double q[3], double& v, double& w) {
    const double a[3] = {static_cast<double>(A.x), static_cast<double>(A.y), static_cast<double>(A.z)};
    const double b[3] = {static_cast<double>(B.x), static_cast<double>(B.y), static_cast<double>(B.z)};
    const double c[3] = {static_cast<double>(C.x), static_cast<double>(C.y), static_cast<double>(C.z)};
    double ab[3], ac[3], x[3];
    for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; x[k] = p[k] - a[k]; }
    const double d1 = dot3(ab, x), d2 = dot3(ac, x);
    v = 0.0; w = 0.0;
    if (d1 <= 0.0 && d2 <= 0.0) { for (int k = 0; k < 3; k++) q[k] = a[k]; return 1; }
    for (int k = 0; k < 3; k++) x[k] = p[k] - b[k];
    const double d3 = dot3(ab, x), d4 = dot3(ac, x);
    if (d3 >= 0.0 && d4 <= d3) { for (int k = 0; k < 3; k++) q[k] = b[k]; v = 1.0; return 2; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        v = d1 / (d1 - d3);
        for (int k = 0; k < 3; k++) q[k] = a[k] + ab[k] * v;
        return 4;
    }
    for (int k = 0; k < 3; k++) x[k] = p[k] - c[k];
    const double d5 = dot3(ab, x), d6 = dot3(ac, x);
    if (d6 >= 0.0 && d5 <= d6) { for (int k = 0; k < 3; k++) q[k] = c[k]; w = 1.0; return 3; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        w = d2 / (d2 - d6);
        for (int k = 0; k < 3; k++) q[k] = a[k] + ac[k] * w;
        return 5;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int k = 0; k < 3; k++) q[k] = b[k] + (c[k] - b[k]) * w;
        v = 1.0 - w;
        return 6;
    }
    const double denom = 1.0 / (va + vb + vc);
    v = vb * denom;
    w = vc * denom;
    for (int k = 0; k < 3; k++) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
    return 0;
}

// the 64 bytes of a record as eight 8-byte stores (the record is 8-byte aligned, no more)
__device__ inline void closest_store(const CastIo& io, uint32_t i, int32_t found, int32_t body, int32_t triangle, int32_t region, double distance,
                                     const double pt[3], double v, double w) {
    unsigned long long* const o = reinterpret_cast<unsigned long long*>(io.out + static_cast<uint64_t>(i) * io.out_stride);
    o[0] = static_cast<unsigned long long>(static_cast<uint32_t>(found)) | (static_cast<unsigned long long>(static_cast<uint32_t>(body)) << 32);
    o[1] = static_cast<unsigned long long>(static_cast<uint32_t>(triangle)) | (static_cast<unsigned long long>(static_cast<uint32_t>(region)) << 32);
    o[2] = static_cast<unsigned long long>(__double_as_longlong(distance));
    for (int k = 0; k < 3; k++) o[3 + k] = static_cast<unsigned long long>(__double_as_longlong(pt[k]));
    o[6] = static_cast<unsigned long long>(__double_as_longlong(v));
    o[7] = static_cast<unsigned long long>(__double_as_longlong(w));
}

// A lane = one query.  It walks the tree of its body (the trees of all bodies, lowest first, without a body array), the child with the
// smaller bound first (query_tree.h: tree_walk), and keeps its best by the lexicographic rule.
template <bool kStats>
__global__ __launch_bounds__(256) void bvh_closest_kernel(QueryDev q, QueryBodiesDev t, BvhDev v, CastIo io, uint32_t first) {
    const uint32_t i = first + blockIdx.x * 256u + threadIdx.x;
    if (!(i < io.count && i >= first)) return;   // (i >= first: the last chunk's index may wrap)
    double p[3], max2;
    bool bad;
    uint32_t body;
    const uint32_t* words;
    {
        const double* const src = reinterpret_cast<const double*>(io.in + static_cast<uint64_t>(i) * io.in_stride);
        for (int k = 0; k < 3; k++) p[k] = src[k];
        const double limit = src[3];
        bad = point_query_defect(p, limit) != kPointGood;
        max2 = limit * limit;
        if (record_body(q, t, io.body, i, &body, &words)) bad = true;
    }
    double bd2 = 0.0, bq[3] = {0.0, 0.0, 0.0}, bv = 0.0, bw = 0.0;
    uint32_t bt = kRayNone;
    TreeCounts count;
    int bregion = -1;
    if (!bad) {
        const double e = tree_padding(words, p);
        count = tree_walk<kStats>(
            q, t, v, io.body ? body : 0u, io.body ? body + 1u : t.bodies,
            // may this node be entered?  (every reason to skip one: this file's head)
            [&](const float lo[3], const float hi[3], double& lb) {
                lb = box_bound(p, e, lo, hi);
                if (lb > max2) return false;
                return !(bt != kRayNone && lb > bd2);
            },
            [&](uint32_t id, const float4 A, const float4 B, const float4 C, const float tlo[3], const float thi[3]) {
                const double lb = box_bound(p, e, tlo, thi);
                if (lb > max2 || (bt != kRayNone && lb > bd2)) return;   // counts only with lb <= d2: it cannot beat the best
                double pt[3], cv, cw;
                const int region = tri_closest(p, A, B, C, pt, cv, cw);
                const double w3[3] = {p[0] - pt[0], p[1] - pt[1], p[2] - pt[2]};
                const double d2 = dot3(w3, w3);
                if (lb <= d2 && d2 <= max2 && better(d2, id, bd2, bt)) {
                    bd2 = d2; bt = id; bregion = region; bv = cv; bw = cw;
                    bq[0] = pt[0]; bq[1] = pt[1]; bq[2] = pt[2];
                }
            });
    }
    const double zero[3] = {0.0, 0.0, 0.0};
    if (bad) closest_store(io, i, -1, -1, -1, -1, 0.0, zero, 0.0, 0.0);                 // TETSIM_CLOSEST_INVALID
    else if (bt == kRayNone) closest_store(io, i, 0, -1, -1, -1, 0.0, zero, 0.0, 0.0);
    else closest_store(io, i, 1, io.body ? static_cast<int32_t>(body) : t.tri_body ? t.tri_body[bt] : 0, static_cast<int32_t>(bt), bregion, sqrt(bd2), bq, bv, bw);
    if (kStats) tree_store_counts(v, i, count);
}

}  // namespace

void query_launch_closest_bvh(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const BvhDev& v, const CastIo& io) {
    launch_per_lane(s, bvh_closest_kernel<false>, bvh_closest_kernel<kTreeCounts>, q, b, v, io);
}

}  // namespace tetsim
