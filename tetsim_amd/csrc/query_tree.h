// query_tree.h -- the one walk of the refitted tree (query_device.h: the layout) behind the range sensors (query_bvh.hip) and the closest
// points (query_closest.hip), and the launch of one lane per record.  Both answers are DEFINED without the tree, and every test a walk
// skips on is monotone in the box, so that tree shape and visit order cannot change a bit of them:
//   * a node's f32 box is tested by the formulas, and with the padding e (tree_padding), of a triangle's own box, and the test only gets
//     easier to pass as the box grows: a box that contains a triangle's box passes whatever the triangle's passes;
//   * a node is skipped only if it holds no triangle or the caller's `open` refuses it, and `open` refuses only what no triangle inside
//     could pass or win (each kernel's head says why for its own predicate; a tie with the best is entered: a lower triangle index may win);
//   * at a leaf every triangle is handed over with the box of its OWN corners, and the caller tests that box again before the triangle.
// The kernels differ in three things: `open`, the key that orders two children (the smaller first), and what is done with a triangle.
#pragma once
#include "dev_common.h"
#include "query_device.h"
#include "query_rays.h"

#include <algorithm>

namespace tetsim {

// include/tetsim.h, "padded box": e = 2^-20 (radius + |x - centre|) of the sphere whose keys are `words`
__device__ inline double tree_padding(const uint32_t* words, const double x[3]) {
    double cen[3], w[3];
    sphere_centre(words, cen);
    const double radius = sphere_radius(words);
    for (int k = 0; k < 3; k++) w[k] = x[k] - cen[k];
    return 0x1p-20 * (radius + sqrt(dot3(w, w)));
}

// what a lane's walk tested (kStats only: TETSIM_BVH_STATS builds)
struct TreeCounts { uint32_t boxes = 0u, tris = 0u; };
__device__ inline void tree_store_counts(const BvhDev& v, uint32_t i, const TreeCounts n) {
    v.stats[2u * static_cast<size_t>(i)] = n.boxes;
    v.stats[2u * static_cast<size_t>(i) + 1u] = n.tris;
}

// A lane walks the trees of the bodies [b0, b1), lowest first.  open(lo, hi, key&) -> may this node be entered, and its key: of two open
// children the one with the smaller key is entered first.  triangle(id, A, B, C, tlo, thi): a triangle of an entered leaf, its corners and
// the box of its own corners.  No stack: going down from a node of level l with both children to visit sets bit l of `pending`; going up,
// the deepest set bit above the node names the ancestor whose other child is next.  (A sibling that waited was opened against an older
// best: the caller's test of a triangle's own box meets the current one.)  Lanes of a wave diverge as their records do; which bodies they
// name costs no more than that.
template <bool kStats, class Open, class Triangle>
__device__ __forceinline__ TreeCounts tree_walk(const QueryDev& q, const QueryBodiesDev& t, const BvhDev& v, uint32_t b0, uint32_t b1, Open open, Triangle triangle) {
    TreeCounts count;
    auto enter = [&](const float lo[3], const float hi[3], double& key) {
        if (lo[0] > hi[0]) return false;   // the empty box: no triangle below
        if (kStats) count.boxes++;
        return open(lo, hi, key);
    };
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t tfirst = t.tri_first[b], ntri = t.tri_first[b + 1u] - tfirst;
        if (ntri == 0u) continue;
        const uint32_t depth = v.depth[b];
        const BvhBox* const box = v.box + v.node_first[b];
        uint32_t node = 1u, pending = 0u;
        bool walking;
        {
            const BvhBox root = box[1];
            double key;
            walking = enter(root.lo, root.hi, key);
        }
        // this subtree is done: up to the deepest ancestor whose other child waits; false: the tree is done
        auto ascend = [&]() {
            const uint32_t level = bvh_level(node), above = pending & ((1u << level) - 1u);
            if (above == 0u) return false;
            const uint32_t l = bvh_level(above);
            pending &= ~(1u << l);
            node = (node >> (level - (l + 1u))) ^ 1u;
            return true;
        };
        while (walking) {
            // Inner nodes first, down to a leaf: a wave leaves this loop when every lane has a leaf or is done, so that the lanes
            // gather and test their leaves' triangles together and not one lane's leaf in every round of the others' descent.
            while (walking && bvh_level(node) < depth) {
                // both children at once: 48 contiguous bytes, 16-byte aligned (node_first is even)
                const float4* const p = reinterpret_cast<const float4*>(box + 2u * node);
                const float4 x = p[0], m = p[1], z = p[2];
                const float lo0[3] = {x.x, x.y, x.z}, hi0[3] = {x.w, m.x, m.y}, lo1[3] = {m.z, m.w, z.x}, hi1[3] = {z.y, z.z, z.w};
                double key0, key1;
                const bool go0 = enter(lo0, hi0, key0), go1 = enter(lo1, hi1, key1);
                if (go0 && go1) { pending |= 1u << bvh_level(node); node = 2u * node + (key1 < key0 ? 1u : 0u); }
                else if (go0 || go1) node = 2u * node + (go1 ? 1u : 0u);
                else walking = ascend();
            }
            if (!walking) break;
            // the leaf's triangles: ids, corners' rows and corners each in one round of loads (an entered leaf holds a triangle: lo < ntri)
            const uint32_t lo = (node - (1u << depth)) * kBvhLeaf, n = ntri - lo < kBvhLeaf ? ntri - lo : kBvhLeaf;
            uint32_t id[kBvhLeaf];
            int4 at[kBvhLeaf];
            float4 A[kBvhLeaf], B[kBvhLeaf], C[kBvhLeaf];
#pragma unroll
            for (uint32_t j = 0; j < kBvhLeaf; j++) id[j] = v.order[tfirst + lo + (j < n ? j : 0u)];   // (behind the end: the first again, not tested)
#pragma unroll
            for (uint32_t j = 0; j < kBvhLeaf; j++) at[j] = q.tri[id[j]];
#pragma unroll
            for (uint32_t j = 0; j < kBvhLeaf; j++) { A[j] = q.pos[at[j].x]; B[j] = q.pos[at[j].y]; C[j] = q.pos[at[j].z]; }
#pragma unroll
            for (uint32_t j = 0; j < kBvhLeaf; j++) {
                if (j >= n) continue;
                float tlo[3] = {INFINITY, INFINITY, INFINITY}, thi[3] = {-INFINITY, -INFINITY, -INFINITY};
                box_add(tlo, thi, A[j]); box_add(tlo, thi, B[j]); box_add(tlo, thi, C[j]);
                if (kStats) count.tris++;
                triangle(id[j], A[j], B[j], C[j], tlo, thi);
            }
            walking = ascend();
        }
    }
    return count;
}

// One lane per record, 256 to a workgroup: `plain` or, where a development build counts (BvhDev::stats), `counting` -- callers name
// kernel<false> and kernel<kTreeCounts>, so that a product build instantiates no counting kernel.
#ifdef TETSIM_BVH_STATS
constexpr bool kTreeCounts = true;
#else
constexpr bool kTreeCounts = false;
#endif
using TreeKernel = void (*)(QueryDev, QueryBodiesDev, BvhDev, CastIo, uint32_t);
inline void launch_per_lane(hipStream_t s, TreeKernel plain, TreeKernel counting, const QueryDev& q, const QueryBodiesDev& b, const BvhDev& v, const CastIo& io) {
    const TreeKernel kernel = v.stats ? counting : plain;
    // a dispatch holds at most 2^32 - 1 work-items (max_grid_blocks)
    const uint64_t chunk = static_cast<uint64_t>(max_grid_blocks(256u)) * 256u;
    for (uint64_t first = 0; first < io.count; first += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, io.count - first);
        hipLaunchKernelGGL(kernel, dim3(static_cast<uint32_t>((n + 255u) / 256u)), dim3(256), 0, s, q, b, v, io, static_cast<uint32_t>(first));
    }
}

}  // namespace tetsim
