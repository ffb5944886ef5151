// query_bvh.hip -- range sensors through a refitted bounding-volume hierarchy (include/tetsim.h: tetsim_raycast_visual_bvh_device;
// query_device.h: the layout; query_tree.h: the walk, and why tree shape and visit order cannot change a bit of the answer).  The answer is
// DEFINED without the tree (tests/raycast_bvh_ref.py is the definition in numpy: brute force with two extra predicates per triangle).
// This walk's predicate:
//   * the padded slab test: a box that contains a triangle's box has tn <= the triangle's tn, tf >= its tf, and passes every axis test
//     the triangle's passes;
//   * a node is refused only if its own test fails, tn > far, tf < near, or a best hit exists and tn > its distance (tn == best is
//     entered: a lower triangle index may tie);
//   * a triangle is tested against the box of its OWN corners, then by tri_test (query_rays.h, the brute-force call's).
// f64, every operation rounded separately: build with -ffp-contract=off.
//   Topology: once per handle on the host (bvh_build_topology, plain C++).  Refit: every call, two launches whatever the batch.
//   Traversal: one lane per ray, stackless -- a complete tree in heap order needs one word of "the sibling is still to do" bits.
#include "dev_common.h"
#include "query_device.h"
#include "query_rays.h"
#include "query_tree.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace tetsim {
namespace {

constexpr uint32_t kFoldLeaves = 1u << kBvhFoldLevels;
static_assert(kFoldLeaves == 256u, "a lane of the fold kernel is one leaf");

__device__ inline BvhBox box_join(const BvhBox& a, const BvhBox& b) {
    BvhBox o;
    for (int k = 0; k < 3; k++) { o.lo[k] = b.lo[k] < a.lo[k] ? b.lo[k] : a.lo[k]; o.hi[k] = b.hi[k] > a.hi[k] ? b.hi[k] : a.hi[k]; }
    return o;
}

// Refit, pass 1.  Workgroup w folds subtree fold[w] = (body, k): a lane = one leaf slot -- the exact f32 min / max of its triangles'
// corners --, then level after level through LDS up to the subtree's root; every box goes to global memory as it is made.  A body of at
// most 256 leaf slots is one subtree, and done; a larger one has 2^(depth - 8) of them, whose roots bvh_top_kernel joins.
__global__ __launch_bounds__(256) void bvh_fold_kernel(QueryDev q, QueryBodiesDev t, BvhDev v) {
    __shared__ BvhBox s_box[kFoldLeaves];
    const uint32_t b = v.fold[2u * blockIdx.x], k = v.fold[2u * blockIdx.x + 1u];
    const uint32_t first = t.tri_first[b], ntri = t.tri_first[b + 1u] - first;
    const uint32_t depth = v.depth[b], levels = depth < kBvhFoldLevels ? depth : kBvhFoldLevels, width = 1u << levels;
    BvhBox* const box = v.box + v.node_first[b];
    const uint32_t leaf = k * width + threadIdx.x;
    BvhBox mine;
    for (int c = 0; c < 3; c++) { mine.lo[c] = INFINITY; mine.hi[c] = -INFINITY; }
    if (threadIdx.x < width) {
        const uint32_t lo = leaf * kBvhLeaf < ntri ? leaf * kBvhLeaf : ntri, hi = lo + kBvhLeaf < ntri ? lo + kBvhLeaf : ntri;   // (leaf < 2^30)
        for (uint32_t j = lo; j < hi; j++) {
            const int4 id = q.tri[v.order[first + j]];
            box_add(mine.lo, mine.hi, q.pos[id.x]);
            box_add(mine.lo, mine.hi, q.pos[id.y]);
            box_add(mine.lo, mine.hi, q.pos[id.z]);
        }
        box[(1u << depth) + leaf] = mine;
    }
    s_box[threadIdx.x] = mine;
    for (uint32_t l = levels; l-- > 0u;) {   // the 2^l nodes of the subtree's level l from the 2^(l + 1) below
        const uint32_t n = 1u << l;
        __syncthreads();
        if (threadIdx.x < n) mine = box_join(s_box[2u * threadIdx.x], s_box[2u * threadIdx.x + 1u]);
        __syncthreads();
        if (threadIdx.x < n) {
            s_box[threadIdx.x] = mine;
            box[(1u << (depth - levels + l)) + k * n + threadIdx.x] = mine;
        }
    }
}

// Refit, pass 2: a workgroup per body of more than 256 leaf slots joins the subtrees' roots, level after level, in global memory (the
// barrier orders a level's stores before the next level's loads within the workgroup).
__global__ __launch_bounds__(256) void bvh_top_kernel(BvhDev v) {
    const uint32_t b = v.top_body[blockIdx.x], depth = v.depth[b];
    BvhBox* const box = v.box + v.node_first[b];
    for (uint32_t l = depth - kBvhFoldLevels; l-- > 0u;) {
        for (uint32_t i = (1u << l) + threadIdx.x; i < (2u << l); i += 256u) box[i] = box_join(box[2u * i], box[2u * i + 1u]);
        __syncthreads();
    }
}

// The ray as the slab test wants it: 1 / d per axis, which axes have none (d == 0, or so small that 1 / d is infinite), the padding.
struct SlabRay { double inv[3]; double e; uint32_t flat; };
// include/tetsim.h, "padded box" and "slab interval": true iff every axis passes and tn <= tf
__device__ inline bool slab_test(const RayPrep& r, const SlabRay& y, const float lo[3], const float hi[3], double& tn, double& tf) {
    tn = -INFINITY; tf = INFINITY;
    for (int k = 0; k < 3; k++) {
        const double L = static_cast<double>(lo[k]) - y.e, H = static_cast<double>(hi[k]) + y.e;
        if (y.flat >> k & 1u) {
            if (!(L <= r.o[k] && r.o[k] <= H)) return false;
        } else {
            const double t1 = (L - r.o[k]) * y.inv[k], t2 = (H - r.o[k]) * y.inv[k];
            const double mn = t1 < t2 ? t1 : t2, mx = t1 > t2 ? t1 : t2;
            tn = mn > tn ? mn : tn;
            tf = mx < tf ? mx : tf;
        }
    }
    return tn <= tf;
}

// A lane = one ray.  It walks the tree of its body (the trees of all bodies, lowest first, without a body array) near child first
// (query_tree.h: tree_walk) and keeps its best by the lexicographic rule.
template <bool kStats>
__global__ __launch_bounds__(256) void bvh_cast_kernel(QueryDev q, QueryBodiesDev t, BvhDev v, CastIo io, uint32_t first) {
    const uint32_t i = first + blockIdx.x * 256u + threadIdx.x;
    if (!(i < io.count && i >= first)) return;   // (i >= first: the last chunk's index may wrap)
    const CastRay c = cast_load(q, t, io, i);
    double bd = 0.0, bp[3] = {0.0, 0.0, 0.0};
    uint32_t bt = kRayNone;
    TreeCounts count;
    RayPrep r;
    r.culled = 1u;
    if (!c.bad) r = ray_prepare(c.r, c.words);
    if (!r.culled) {
        SlabRay y;
        y.e = tree_padding(c.words, r.o);
        y.flat = 0u;
        for (int k = 0; k < 3; k++) {
            y.inv[k] = 1.0 / r.d[k];
            if (r.d[k] == 0.0 || y.inv[k] - y.inv[k] != 0.0) y.flat |= 1u << k;   // (x - x: NaN for an infinity)
        }
        count = tree_walk<kStats>(
            q, t, v, io.body ? c.body : 0u, io.body ? c.body + 1u : t.bodies,
            // may this node be entered?  (every reason to skip one: this file's head)
            [&](const float lo[3], const float hi[3], double& tn) {
                double tf;
                if (!slab_test(r, y, lo, hi, tn, tf)) return false;
                if (tn > r.far || tf < r.near) return false;
                return !(bt != kRayNone && tn > bd);
            },
            [&](uint32_t id, const float4 A, const float4 B, const float4 C, const float tlo[3], const float thi[3]) {
                double tn, tf, d, pt[3];
                if (!slab_test(r, y, tlo, thi, tn, tf)) return;           // not a candidate
                if (tri_hit(r, A, B, C, d, pt) && tn <= d && d <= tf && better(d, id, bd, bt)) {
                    bd = d; bt = id;
                    bp[0] = pt[0]; bp[1] = pt[1]; bp[2] = pt[2];
                }
            });
    }
    cast_store_result(t, io, i, c, bt, bd, bp);
    if (kStats) tree_store_counts(v, i, count);
}

// 10 bits per axis, interleaved
uint32_t morton30(const uint32_t q[3]) {
    uint32_t code = 0;
    for (int bit = 9; bit >= 0; bit--)
        for (int k = 0; k < 3; k++) code = code << 1 | (q[k] >> bit & 1u);
    return code;
}

}  // namespace

std::string bvh_build_topology(const float* pos, uint32_t pos_stride, const int32_t* tri, uint32_t tri_stride, const uint32_t* tri_sorted,
                               const uint32_t* tri_first, uint32_t bodies, BvhTopology* out) {
    const uint32_t ntri = tri_first[bodies];
    out->order.assign(tri_sorted, tri_sorted + ntri);
    out->node_first.assign(bodies + 1u, 0u);
    out->depth.assign(bodies, 0u);
    out->fold.clear();
    out->top_body.clear();
    std::vector<uint32_t> code(ntri);
    uint64_t nodes = 0;
    for (uint32_t b = 0; b < bodies; b++) {
        const uint32_t lo = tri_first[b], hi = tri_first[b + 1u], n = hi - lo;
        // the centroids in the box of the body's triangles, 10 bits per axis (a centroid that is not finite sorts first)
        float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        std::vector<float> cen(3ull * n);
        for (uint32_t j = 0; j < n; j++) {
            const int32_t* const at = tri + static_cast<size_t>(tri_stride) * tri_sorted[lo + j];
            for (int k = 0; k < 3; k++) {
                const float c = (pos[static_cast<size_t>(pos_stride) * at[0] + k] + pos[static_cast<size_t>(pos_stride) * at[1] + k] +
                                 pos[static_cast<size_t>(pos_stride) * at[2] + k]) / 3.0f;
                cen[3ull * j + k] = c;
                if (c < blo[k]) blo[k] = c;
                if (c > bhi[k]) bhi[k] = c;
            }
        }
        for (uint32_t j = 0; j < n; j++) {
            uint32_t qk[3];
            for (int k = 0; k < 3; k++) {
                const float ext = bhi[k] - blo[k], x = ext > 0.0f ? (cen[3ull * j + k] - blo[k]) / ext : 0.0f;
                qk[k] = x > 0.0f ? std::min(1023u, static_cast<uint32_t>(x * 1024.0f)) : 0u;   // (x > 0 is false for a NaN)
            }
            code[lo + j] = morton30(qk);
        }
        // by (code, triangle id): tri_sorted is ascending inside a body, so a stable sort by code is that order
        std::vector<uint32_t> at(n);
        std::iota(at.begin(), at.end(), 0u);
        std::stable_sort(at.begin(), at.end(), [&](uint32_t x, uint32_t y) { return code[lo + x] < code[lo + y]; });
        for (uint32_t j = 0; j < n; j++) out->order[lo + j] = tri_sorted[lo + at[j]];
        const uint32_t depth = bvh_depth(bvh_leaves(n)), slots = 1u << depth;
        out->depth[b] = depth;
        nodes += 2ull * slots;
        if (nodes > 0x7fffffffull) return "the visual mesh has too many triangles for the tree's 32-bit node offsets";
        out->node_first[b + 1u] = static_cast<uint32_t>(nodes);
        const uint32_t subtrees = depth > kBvhFoldLevels ? 1u << (depth - kBvhFoldLevels) : 1u;
        for (uint32_t k = 0; k < subtrees; k++) { out->fold.push_back(b); out->fold.push_back(k); }
        if (depth > kBvhFoldLevels) out->top_body.push_back(b);
    }
    return "";
}

void query_launch_bvh_refit(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const BvhDev& v) {
    // (folds <= triangles / 1024 + bodies: within a dispatch's 2^32 - 1 work-items for every mesh whose tables fit 32-bit offsets)
    if (v.folds) hipLaunchKernelGGL(bvh_fold_kernel, dim3(v.folds), dim3(256), 0, s, q, b, v);
    if (v.tops) hipLaunchKernelGGL(bvh_top_kernel, dim3(v.tops), dim3(256), 0, s, v);
}

void query_launch_cast_bvh(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const BvhDev& v, const CastIo& io) {
    launch_per_lane(s, bvh_cast_kernel<false>, bvh_cast_kernel<kTreeCounts>, q, b, v, io);
}

}  // namespace tetsim
