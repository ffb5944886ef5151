// query_bvh.hip -- range sensors through a refitted bounding-volume hierarchy (include/tetsim.h: tetsim_raycast_visual_bvh_device;
// query_device.h: the layout).  The answer is DEFINED without the tree (tests/raycast_bvh_ref.py is the definition in numpy: brute force
// with two extra predicates per triangle), and every test the traversal skips on is monotone in the box, so that tree shape and visit
// order cannot change a bit of it:
//   * the padded slab test of a node's f32 box uses the formulas and the padding e of a triangle's own box; a box that contains a
//     triangle's box has tn <= the triangle's tn, tf >= its tf, and passes every axis test the triangle's passes;
//   * a node is skipped only if it holds no triangle, its own test fails, tn > far, tf < near, or a best hit exists and tn > its distance
//     (tn == best is entered: a lower triangle index may tie);
//   * at a leaf every triangle is tested against the box of its OWN corners, then by tri_test (query_rays.h, the brute-force call's).
// f64, every operation rounded separately: build with -ffp-contract=off.
//   Topology: once per handle on the host (bvh_build_topology, plain C++).  Refit: every call, two launches whatever the batch.
//   Traversal: one lane per ray, stackless -- a complete tree in heap order needs one word of "the sibling is still to do" bits.
#include "dev_common.h"
#include "query_device.h"
#include "query_rays.h"

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

// A lane = one ray.  It walks the tree of its body (the trees of all bodies, lowest first, without ray_body) near child first and keeps
// its best by the lexicographic rule.  No stack: going down from a node of level l with both children to visit sets bit l of `pending`;
// going up, the deepest set bit above the node names the ancestor whose other child is next.  Lanes of a wave diverge as their rays do;
// which bodies they name costs no more than that.
template <bool kStats>
__global__ __launch_bounds__(256) void bvh_cast_kernel(QueryDev q, QueryBodiesDev t, BvhDev v, CastIo io, uint32_t first) {
    const uint32_t i = first + blockIdx.x * 256u + threadIdx.x;
    if (!(i < io.count && i >= first)) return;   // (i >= first: the last chunk's index may wrap)
    const CastRay c = cast_load(q, t, io, i);
    double bd = 0.0, bp[3] = {0.0, 0.0, 0.0};
    uint32_t bt = kRayNone, boxes = 0u, tris = 0u;
    RayPrep r;
    r.culled = 1u;
    if (!c.bad) r = ray_prepare(c.r, c.words);
    if (!r.culled) {
        SlabRay y;
        {
            double cen[3], w[3];
            sphere_centre(c.words, cen);
            const double radius = sqrt(__longlong_as_double(static_cast<long long>(*reinterpret_cast<const unsigned long long*>(c.words + 6))));
            for (int k = 0; k < 3; k++) w[k] = r.o[k] - cen[k];
            y.e = 0x1p-20 * (radius + sqrt(dot3(w, w)));
            y.flat = 0u;
            for (int k = 0; k < 3; k++) {
                y.inv[k] = 1.0 / r.d[k];
                if (r.d[k] == 0.0 || y.inv[k] - y.inv[k] != 0.0) y.flat |= 1u << k;   // (x - x: NaN for an infinity)
            }
        }
        // may this node be entered?  (every reason to skip one: query_bvh.hip's head)
        auto open = [&](const float lo[3], const float hi[3], double& tn) {
            if (lo[0] > hi[0]) return false;   // the empty box: no triangle below
            if (kStats) boxes++;
            double tf;
            if (!slab_test(r, y, lo, hi, tn, tf)) return false;
            if (tn > r.far || tf < r.near) return false;
            return !(bt != kRayNone && tn > bd);
        };
        const uint32_t b0 = io.ray_body ? c.body : 0u, b1 = io.ray_body ? c.body + 1u : t.bodies;
        for (uint32_t b = b0; b < b1; b++) {
            const uint32_t tfirst = t.tri_first[b], ntri = t.tri_first[b + 1u] - tfirst;
            if (ntri == 0u) continue;
            const uint32_t depth = v.depth[b];
            const BvhBox* const box = v.box + v.node_first[b];
            uint32_t node = 1u, pending = 0u;
            bool walking;
            {
                const BvhBox root = box[1];
                double tn;
                walking = open(root.lo, root.hi, tn);
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
                    double tn0, tn1;
                    const bool go0 = open(lo0, hi0, tn0), go1 = open(lo1, hi1, tn1);
                    if (go0 && go1) { pending |= 1u << bvh_level(node); node = 2u * node + (tn1 < tn0 ? 1u : 0u); }
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
                    if (kStats) tris++;
                    double tn, tf, d, pt[3];
                    if (!slab_test(r, y, tlo, thi, tn, tf)) continue;           // not a candidate
                    if (tri_hit(r, A[j], B[j], C[j], d, pt) && tn <= d && d <= tf && better(d, id[j], bd, bt)) {
                        bd = d; bt = id[j];
                        bp[0] = pt[0]; bp[1] = pt[1]; bp[2] = pt[2];
                    }
                }
                walking = ascend();
            }
        }
    }
    cast_store_result(t, io, i, c, bt, bd, bp);
    if (kStats) { v.stats[2u * static_cast<size_t>(i)] = boxes; v.stats[2u * static_cast<size_t>(i) + 1u] = tris; }
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
    // a dispatch holds at most 2^32 - 1 work-items (max_grid_blocks)
    const uint64_t chunk = static_cast<uint64_t>(max_grid_blocks(256u)) * 256u;
    for (uint64_t first = 0; first < io.count; first += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, io.count - first);
        const dim3 grid(static_cast<uint32_t>((n + 255u) / 256u));
#ifdef TETSIM_BVH_STATS
        if (v.stats) { hipLaunchKernelGGL(bvh_cast_kernel<true>, grid, dim3(256), 0, s, q, b, v, io, static_cast<uint32_t>(first)); continue; }
#endif
        hipLaunchKernelGGL(bvh_cast_kernel<false>, grid, dim3(256), 0, s, q, b, v, io, static_cast<uint32_t>(first));
    }
}

}  // namespace tetsim
