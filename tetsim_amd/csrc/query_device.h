// query_device.h -- range sensors on the device (include/tetsim.h: tetsim_raycast_visual_device / tetsim_raycast_visual_bvh_device /
// tetsim_visual_bounding_spheres_device): what tetsim_query.hip and the query kernels' units share beyond dev_common.h -- the one definition of
// an invalid ray, the per-body tables of a handle's visual mesh and the launches over them.
#pragma once
#include "dev_common.h"

#include <string>
#include <vector>

namespace tetsim {

// Why a ray is refused, 0 = it is good: the host's check_rays turns the code into TETSIM_EINVAL and a message, the device's cast into
// TETSIM_RAY_INVALID.  o, d: origin and direction.
enum : int { kRayGood = 0, kRayNonFinite, kRayZeroDirection, kRayNanWindow, kRayNegativeNear, kRayFarBelowNear };
__host__ __device__ inline int ray_defect(const double o[3], const double d[3], double near, double far) {
    bool finite = true;
    for (int k = 0; k < 3; k++) finite = finite && (o[k] - o[k] == 0.0) && (d[k] - d[k] == 0.0);   // (x - x: NaN for an infinity or a NaN)
    if (!finite) return kRayNonFinite;
    if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) return kRayZeroDirection;
    if (near != near || far != far) return kRayNanWindow;
    if (near < 0.0) return kRayNegativeNear;
    if (far < near) return kRayFarBelowNear;
    return kRayGood;
}

// The bodies of a handle's visual mesh, built once on the host (tetsim_query.hip: ensure_row_tables / ensure_triangle_tables).
struct QueryBodiesDev {
    uint32_t bodies = 0;
    const uint32_t* row_body = nullptr;     // [nvis] the body whose tets carry the row
    const uint32_t* body_rows = nullptr;    // [bodies] how many rows that is
    uint32_t* spheres = nullptr;            // [bodies][kSphereWords], the keys of QueryDev::sphere per body
    const uint32_t* tri_sorted = nullptr;   // [ntri] triangle ids stably sorted by body: a body's triangles in the caller's list order
    const uint32_t* tri_first = nullptr;    // [bodies + 1] offsets into tri_sorted
    const int32_t* tri_body = nullptr;      // [ntri] the body of a triangle's first vertex (what tetsim_raycast_visual names); null = body 0
    uint32_t max_tiles = 1;                 // tiles of kCastTile triangles of the largest body
};
constexpr uint32_t kCastTile = 256;         // triangles staged in LDS at a time = rays of a workgroup
constexpr uint32_t kCastCandCap = 1u << 17; // candidates of the split launches (few rays): 2 MiB, whatever the count

// The caller's records, of a cast or of a closest-point call (the struct keeps its first user's name): ray or query i at in + i * in_stride,
// its body at body[i] (null: the whole mesh), its hit or answer at out + i * out_stride.
struct CastIo {
    const char* in; uint64_t in_stride;
    const int32_t* body;
    char* out; uint64_t out_stride;
    uint32_t count;
};

// every body's sphere keys into b.spheres (a memset and two reductions keyed by the row's body, in stream order)
void query_launch_body_spheres(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b);
// row k of dst = (centre xyz, radius) of body k, 4 doubles; a body without rows: zeros
void query_launch_spheres_out(hipStream_t s, const QueryBodiesDev& b, char* dst, uint64_t stride);
// The cast: q.sphere (io.body null) or b.spheres (else) must be current.  cand: kCastCandCap entries.
void query_launch_cast_device(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const CastIo& io, RayCand* cand);
// into how many parts the triangle range is split over gridDim.y (few rays must not run on few compute units)
uint32_t query_cast_splits(uint32_t tiles, uint32_t count);

// ---- the refitted tree behind tetsim_raycast_visual_bvh_device (query_bvh.hip) ---------------------------------------------------------
// Per body a COMPLETE BINARY TREE IN HEAP ORDER over its leaves: the body's triangles (its tri_first range) in the Morton order of their
// centroids, kBvhLeaf consecutive ones to a leaf, the leaves padded to a power of two.  Node 1 is the root, node i has the children 2i and
// 2i + 1, the leaves are the nodes [2^depth, 2^(depth + 1)); nothing else is stored: no child or parent pointers, no counters.  A node's
// box is the exact f32 min / max of its triangles' corners; a node without triangles keeps the empty box (lo = +inf > hi = -inf).
constexpr uint32_t kBvhLeaf = 4;            // triangles of a leaf
constexpr uint32_t kBvhFoldLevels = 8;      // levels a workgroup of the refit folds through LDS: 2^8 leaves = its 256 lanes
struct BvhBox { float lo[3], hi[3]; };
struct BvhDev {
    const uint32_t* order = nullptr;        // [ntri] position in a body's tri_first range -> triangle id, the body's Morton order
    const uint32_t* node_first = nullptr;   // [bodies] where the body's nodes start in `box` (even; slot 0 of a body is unused)
    const uint32_t* depth = nullptr;        // [bodies] levels below the root: 2^depth leaf slots
    BvhBox* box = nullptr;                  // [node_first[bodies]]
    const uint32_t* fold = nullptr;         // [folds][2] (body, subtree): what workgroup w of the refit's first pass folds
    const uint32_t* top_body = nullptr;     // [tops] the bodies of more than 2^kBvhFoldLevels leaf slots: the second pass, a workgroup each
    uint32_t folds = 0, tops = 0;
    uint32_t* stats = nullptr;              // development (TETSIM_BVH_STATS builds only): [count][2] boxes and triangles tested per ray
};
__host__ __device__ inline uint32_t bvh_leaves(uint32_t ntri) { return ntri / kBvhLeaf + (ntri % kBvhLeaf ? 1u : 0u); }
__host__ __device__ inline uint32_t bvh_depth(uint32_t leaves) { uint32_t d = 0; while ((1u << d) < leaves) d++; return d; }
__host__ __device__ inline uint32_t bvh_level(uint32_t node) { return 31u - static_cast<uint32_t>(__builtin_clz(node)); }
// the leaves [first, end) below node `node` of a tree of `depth` levels (the padding included: clip with the body's leaf count)
__host__ __device__ inline void bvh_node_leaves(uint32_t node, uint32_t depth, uint32_t* first, uint32_t* end) {
    const uint32_t level = bvh_level(node), span = depth - level;
    *first = (node - (1u << level)) << span;
    *end = *first + (1u << span);
}
// The topology, built once on the host (no device needed: tetsim_prep_bvh returns it).  pos: xyz at pos + pos_stride * row; tri: three
// rows at tri + tri_stride * id; tri_sorted / tri_first as in QueryBodiesDev.  "" or what is wrong.
struct BvhTopology {
    std::vector<uint32_t> order, node_first /* [bodies + 1] */, depth, fold, top_body;
};
std::string bvh_build_topology(const float* pos, uint32_t pos_stride, const int32_t* tri, uint32_t tri_stride, const uint32_t* tri_sorted,
                               const uint32_t* tri_first, uint32_t bodies, BvhTopology* out);
// the refit, in stream order behind the skinning: two launches whatever the number of bodies (the second only if some body has tops)
void query_launch_bvh_refit(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const BvhDev& v);
// The cast: q.sphere (io.body null) or b.spheres (else) and the boxes must be current.
void query_launch_cast_bvh(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const BvhDev& v, const CastIo& io);

// ---- closest-point queries through the same tree (include/tetsim.h: tetsim_closest_visual_device; query_closest.hip) ----------------
struct PointQueryIn { double p[3], max_distance; };                                                   // = TetSimPointQuery
struct ClosestOut { int32_t found, body, triangle, region; double distance, point[3], v, w; };      // = TetSimClosest
// Why a query is refused, 0 = it is good: the host variant turns the code into TETSIM_EINVAL and a message, the device into
// TETSIM_CLOSEST_INVALID.
enum : int { kPointGood = 0, kPointNonFinite, kPointNanLimit, kPointNegativeLimit };
__host__ __device__ inline int point_query_defect(const double p[3], double max_distance) {
    for (int k = 0; k < 3; k++)
        if (!(p[k] - p[k] == 0.0)) return kPointNonFinite;   // (x - x: NaN for an infinity or a NaN)
    if (max_distance != max_distance) return kPointNanLimit;
    if (max_distance < 0.0) return kPointNegativeLimit;
    return kPointGood;
}
// The queries (io: CastIo above): q.sphere (io.body null) or b.spheres (else) and the boxes must be current.
void query_launch_closest_bvh(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const BvhDev& v, const CastIo& io);

}  // namespace tetsim
