// query_device.h -- range sensors on the device (include/tetsim.h: tetsim_raycast_visual_device /
// tetsim_visual_bounding_spheres_device): what tetsim_visual.hip and query_kernels.hip share beyond dev_common.h -- the one definition of
// an invalid ray, the per-body tables of a handle's visual mesh and the launches over them.
#pragma once
#include "dev_common.h"

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

// The bodies of a handle's visual mesh, built once on the host (tetsim_visual.hip: ensure_row_tables / ensure_triangle_tables).
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

// the caller's records: ray i at rays + i * ray_stride, its body at ray_body[i] (null: the whole mesh), its hit at hits + i * hit_stride
struct CastIo {
    const char* rays; uint64_t ray_stride;
    const int32_t* ray_body;
    char* hits; uint64_t hit_stride;
    uint32_t count;
};

// every body's sphere keys into b.spheres (a memset and two reductions keyed by the row's body, in stream order)
void query_launch_body_spheres(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b);
// row k of dst = (centre xyz, radius) of body k, 4 doubles; a body without rows: zeros
void query_launch_spheres_out(hipStream_t s, const QueryBodiesDev& b, char* dst, uint64_t stride);
// The cast: q.sphere (io.ray_body null) or b.spheres (else) must be current.  cand: kCastCandCap entries.
void query_launch_cast_device(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const CastIo& io, RayCand* cand);
// into how many parts the triangle range is split over gridDim.y (few rays must not run on few compute units)
uint32_t query_cast_splits(uint32_t tiles, uint32_t count);

}  // namespace tetsim
