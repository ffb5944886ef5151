// query_kernels.hip -- picking on the device: three.js r160 ray casts against the skinned visual mesh and its bounding sphere.
// Reference: Grabber.start / GPUGrabber.start (Softbody.js:440-456, SoftbodyGPU.js:788-811) cast the pointer's ray with three's
// Raycaster after reading the mesh back; endFrame ends with geometry.computeBoundingSphere() (Softbody.js:256,276).  Restated
// from three's Mesh.raycast, checkGeometryIntersection, Ray.intersectTriangle and BufferGeometry.computeBoundingSphere:
//   * f64 arithmetic on the f32 positions, every operation rounded separately, sums left to right -- build with
//     -ffp-contract=off; the result equals JavaScript's bit for bit (tests/raycast_ref.py is the same text in numpy);
//   * brute force: every ray against every triangle.  The winner is the smallest (distance, triangle index) in lexicographic
//     order at every level of the reduction, so it depends neither on the grid shape nor on scheduling; no floating-point atomics.
//   * the sphere: min / max of f32 values and the max of non-negative f64 values are order-free, so integer atomicMax on
//     order-preserving keys gives the same bits whatever the order.
#include "dev_common.h"
#include "query_device.h"
#include "query_rays.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace tetsim {
namespace {

__global__ __launch_bounds__(256) void sphere_minmax_kernel(const float4* __restrict__ pos, uint32_t n, uint32_t* __restrict__ words) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const float4 p = pos[i];
        const float v[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; k++) { lo[k] = v[k] < lo[k] ? v[k] : lo[k]; hi[k] = v[k] > hi[k] ? v[k] : hi[k]; }
    }
    for (int k = 0; k < 3; k++)
        for (int m = 32; m > 0; m >>= 1) {
            const float a = __shfl_xor(lo[k], m, 64), b = __shfl_xor(hi[k], m, 64);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    if ((threadIdx.x & 63u) == 0u && hi[0] >= lo[0])   // (a wave that saw no vertex has nothing to say)
        for (int k = 0; k < 3; k++) {
            atomicMax(&words[k], ~key_of(__float_as_uint(lo[k])));
            atomicMax(&words[3 + k], key_of(__float_as_uint(hi[k])));
        }
}

// maxRadiusSq = max_i center.distanceToSquared(p_i): dx = centre.x - p.x; dx*dx + dy*dy + dz*dz
__global__ __launch_bounds__(256) void sphere_radius_kernel(const float4* __restrict__ pos, uint32_t n, uint32_t* __restrict__ words) {
    double c[3];
    sphere_centre(words, c);
    double best = 0.0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const float4 p = pos[i];
        const double dx = c[0] - static_cast<double>(p.x), dy = c[1] - static_cast<double>(p.y), dz = c[2] - static_cast<double>(p.z);
        const double d2 = dx * dx + dy * dy + dz * dz;
        best = d2 > best ? d2 : best;
    }
    for (int m = 32; m > 0; m >>= 1) {
        const double o = __shfl_xor(best, m, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63u) == 0u)   // non-negative doubles order like their bit patterns
        atomicMax(reinterpret_cast<unsigned long long*>(words + 6), static_cast<unsigned long long>(__double_as_longlong(best)));
}

__global__ __launch_bounds__(256) void ray_prep_kernel(const RayIn* __restrict__ rays, uint32_t count, const uint32_t* __restrict__ words, RayPrep* __restrict__ prep) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    prep[i] = ray_prepare(rays[i], words);
}

__device__ inline void wave_best(double& d, uint32_t& t) {
    for (int m = 32; m > 0; m >>= 1) {
        const double od = __shfl_xor(d, m, 64);
        const uint32_t ot = __shfl_xor(t, m, 64);
        if (better(od, ot, d, t)) { d = od; t = ot; }
    }
}

// grid = (blocks per ray, rays): a lane walks its triangles with a grid stride and keeps its best; one candidate per block.
// The ray's record is the same for the whole block: the compiler keeps it in scalar registers (uniform loads).
__global__ __launch_bounds__(256) void ray_triangles_kernel(QueryDev q, const RayPrep* __restrict__ prep, RayCand* __restrict__ cand) {
    __shared__ double s_d[4];
    __shared__ uint32_t s_t[4];
    const RayPrep r = prep[blockIdx.y];
    double bd = 0.0;
    uint32_t bt = kRayNone;
    if (!r.culled)
        for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < q.ntri; t += gridDim.x * 256u) {
            const int4 id = q.tri[t];
            double d, pt[3];
            if (tri_hit(r, q.pos[id.x], q.pos[id.y], q.pos[id.z], d, pt) && better(d, t, bd, bt)) { bd = d; bt = t; }
        }
    wave_best(bd, bt);
    if ((threadIdx.x & 63u) == 0u) { s_d[threadIdx.x >> 6] = bd; s_t[threadIdx.x >> 6] = bt; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (int w = 1; w < 4; w++)
            if (better(s_d[w], s_t[w], bd, bt)) { bd = s_d[w]; bt = s_t[w]; }
        RayCand c;
        c.distance = bd; c.triangle = bt; c.pad = 0u;
        cand[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = c;
    }
}

// one wave per ray: the smallest of its candidates, then the record (the winner's point is computed again, by the same code)
__global__ __launch_bounds__(256) void ray_pick_kernel(QueryDev q, const RayPrep* __restrict__ prep, const RayCand* __restrict__ cand, uint32_t per_ray,
                                                       uint32_t count, RayOut* __restrict__ hits) {
    const uint32_t ray = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (ray >= count) return;
    double bd = 0.0;
    uint32_t bt = kRayNone;
    for (uint32_t c = lane; c < per_ray; c += 64u) {
        const RayCand k = cand[static_cast<size_t>(ray) * per_ray + c];
        if (better(k.distance, k.triangle, bd, bt)) { bd = k.distance; bt = k.triangle; }
    }
    wave_best(bd, bt);
    if (lane != 0u) return;
    RayOut o;
    o.hit = 0; o.body = -1; o.triangle = -1; o.reserved = 0; o.distance = 0.0; o.point[0] = o.point[1] = o.point[2] = 0.0;
    if (bt != kRayNone) {
        const RayPrep r = prep[ray];
        const int4 id = q.tri[bt];
        double d, pt[3];
        if (tri_hit(r, q.pos[id.x], q.pos[id.y], q.pos[id.z], d, pt)) {
            o.hit = 1; o.body = 0; o.triangle = static_cast<int32_t>(bt); o.distance = d;
            o.point[0] = pt[0]; o.point[1] = pt[1]; o.point[2] = pt[2];
        }
    }
    hits[ray] = o;
}

// ---- range sensors (query_device.h): rays, their bodies and the hits in the caller's device memory -----------------------------------

// The two sphere reductions keyed by the row's body: a lane = one row.  Rows of one body usually follow each other, so a wave whose
// rows share a body reduces first and issues one set of atomics; a mixed wave issues them per lane.  Order-free either way.
__global__ __launch_bounds__(256) void body_sphere_minmax_kernel(const float4* __restrict__ pos, const uint32_t* __restrict__ row_body, uint32_t n,
                                                                 uint32_t* __restrict__ words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, row = i < n ? i : n - 1u;   // (n > 0; a lane behind the end keeps the last row's body and says nothing)
    const uint32_t b = row_body[row];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        const float4 p = pos[i];
        const float v[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; k++) { lo[k] = v[k] < lo[k] ? v[k] : lo[k]; hi[k] = v[k] > hi[k] ? v[k] : hi[k]; }
    }
    const bool uniform = __all(b == __shfl(b, 0, 64));
    if (uniform)
        for (int k = 0; k < 3; k++)
            for (int m = 32; m > 0; m >>= 1) {
                const float a = __shfl_xor(lo[k], m, 64), c = __shfl_xor(hi[k], m, 64);
                lo[k] = a < lo[k] ? a : lo[k];
                hi[k] = c > hi[k] ? c : hi[k];
            }
    // (a wave of one body speaks as a wave of sphere_minmax_kernel does; in a mixed wave every live lane speaks for its row, and a NaN
    // component's infinities change no key.  With non-finite positions the existing reduction already depends on which rows share a wave.)
    if (uniform ? ((threadIdx.x & 63u) == 0u && hi[0] >= lo[0]) : i < n) {
        uint32_t* const w = words + static_cast<size_t>(b) * kSphereWords;
        for (int k = 0; k < 3; k++) {
            atomicMax(&w[k], ~key_of(__float_as_uint(lo[k])));
            atomicMax(&w[3 + k], key_of(__float_as_uint(hi[k])));
        }
    }
}

__global__ __launch_bounds__(256) void body_sphere_radius_kernel(const float4* __restrict__ pos, const uint32_t* __restrict__ row_body, uint32_t n,
                                                                 uint32_t* __restrict__ words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, row = i < n ? i : n - 1u;
    const uint32_t b = row_body[row];
    uint32_t* const w = words + static_cast<size_t>(b) * kSphereWords;
    double best = 0.0;
    if (i < n) {
        double c[3];
        sphere_centre(w, c);
        const float4 p = pos[i];
        const double dx = c[0] - static_cast<double>(p.x), dy = c[1] - static_cast<double>(p.y), dz = c[2] - static_cast<double>(p.z);
        const double d2 = dx * dx + dy * dy + dz * dz;
        best = d2 > best ? d2 : best;
    }
    const bool uniform = __all(b == __shfl(b, 0, 64));
    if (uniform)
        for (int m = 32; m > 0; m >>= 1) {
            const double o = __shfl_xor(best, m, 64);
            best = o > best ? o : best;
        }
    if (!uniform || (threadIdx.x & 63u) == 0u)
        atomicMax(reinterpret_cast<unsigned long long*>(w + 6), static_cast<unsigned long long>(__double_as_longlong(best)));
}

// a lane = one body: its keys decoded as query_decode_sphere does; only the 32 bytes of the row are written
__global__ __launch_bounds__(256) void body_spheres_out_kernel(const uint32_t* __restrict__ words, const uint32_t* __restrict__ body_rows, uint32_t bodies,
                                                               char* __restrict__ dst, uint64_t stride) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= bodies) return;
    double* const o = reinterpret_cast<double*>(dst + static_cast<uint64_t>(b) * stride);
    if (body_rows[b] == 0u) { o[0] = o[1] = o[2] = o[3] = 0.0; return; }   // three's empty Box3: centre 0, radius 0
    const uint32_t* const w = words + static_cast<size_t>(b) * kSphereWords;
    double c[3];
    sphere_centre(w, c);
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    o[3] = sphere_radius(w);
}

// A lane = one ray, a workgroup = kCastTile rays; grid = (workgroups of rays, parts of the triangle range).  The workgroup goes through
// the bodies its rays name, lowest first (one body when the rays are grouped by body, the fast case; the whole mesh without ray_body):
// every lane prepares one triangle of the tile into LDS (tri_prepare: the gathers and the f64 conversions happen once per triangle and
// workgroup, not once per ray), then the lanes whose ray belongs to that body read the same prepared record one after the other -- an
// LDS broadcast -- and keep their best by the lexicographic rule.  kSplit: part y takes tiles y, y + gridDim.y, ..; its best goes to
// cand[y * count + ray] and cast_finish_kernel picks; otherwise the record is written here.
template <bool kSplit>
__global__ __launch_bounds__(256) void cast_device_kernel(QueryDev q, QueryBodiesDev t, CastIo io, uint32_t first, RayCand* __restrict__ cand) {
    __shared__ TriRec s_tri[kCastTile];
    __shared__ uint32_t s_id[kCastTile];
    __shared__ uint32_t s_next;
    const uint32_t i = first + blockIdx.x * kCastTile + threadIdx.x;
    const bool live = i < io.count && i >= first;   // (i >= first: the last chunk's index may wrap)
    CastRay c;
    RayPrep r;
    bool todo = false;
    if (live) {
        c = cast_load(q, t, io, i);
        if (!c.bad) { r = ray_prepare(c.r, c.words); todo = !r.culled; }
    }
    double bd = 0.0, bp[3] = {0.0, 0.0, 0.0};
    uint32_t bt = kRayNone;
    for (;;) {
        if (threadIdx.x == 0u) s_next = kRayNone;
        __syncthreads();
        if (todo) atomicMin(&s_next, c.body);
        __syncthreads();
        const uint32_t cur = s_next;      // the same for the whole workgroup: every barrier below is reached by all of it
        if (cur == kRayNone) break;
        const bool mine = todo && c.body == cur;
        const uint64_t lo = io.body ? t.tri_first[cur] : 0u, hi = io.body ? t.tri_first[cur + 1u] : q.ntri;
        for (uint64_t base = lo + static_cast<uint64_t>(blockIdx.y) * kCastTile; base < hi; base += static_cast<uint64_t>(gridDim.y) * kCastTile) {
            __syncthreads();              // (the tile before this one has been read)
            const uint64_t k = base + threadIdx.x;
            if (k < hi) {
                const uint32_t id = io.body ? t.tri_sorted[k] : static_cast<uint32_t>(k);
                const int4 v = q.tri[id];
                tri_prepare(q.pos[v.x], q.pos[v.y], q.pos[v.z], s_tri[threadIdx.x]);
                s_id[threadIdx.x] = id;
            }
            __syncthreads();
            if (mine) {
                const uint32_t n = hi - base < kCastTile ? static_cast<uint32_t>(hi - base) : kCastTile;
                for (uint32_t j = 0; j < n; j++) {
                    double d, pt[3];
                    if (tri_test(r, s_tri[j].a, s_tri[j].e1, s_tri[j].e2, s_tri[j].n, d, pt) && better(d, s_id[j], bd, bt)) {
                        bd = d; bt = s_id[j];
                        bp[0] = pt[0]; bp[1] = pt[1]; bp[2] = pt[2];
                    }
                }
            }
        }
        if (mine) todo = false;
        __syncthreads();                  // (everybody has read s_next)
    }
    if (!live) return;
    if (kSplit) {
        RayCand k;
        k.distance = bd; k.triangle = bt; k.pad = 0u;
        cand[static_cast<size_t>(blockIdx.y) * io.count + i] = k;
    } else {
        cast_store_result(t, io, i, c, bt, bd, bp);
    }
}

// split launches: a lane = one ray; the smallest of its parts' candidates, then the record (the winner's point is computed again, by the same code)
__global__ __launch_bounds__(256) void cast_finish_kernel(QueryDev q, QueryBodiesDev t, CastIo io, const RayCand* __restrict__ cand, uint32_t parts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= io.count) return;
    const CastRay c = cast_load(q, t, io, i);
    double bd = 0.0, bp[3] = {0.0, 0.0, 0.0};
    uint32_t bt = kRayNone;
    for (uint32_t p = 0; p < parts; p++) {
        const RayCand k = cand[static_cast<size_t>(p) * io.count + i];
        if (better(k.distance, k.triangle, bd, bt)) { bd = k.distance; bt = k.triangle; }
    }
    if (!c.bad && bt != kRayNone) {
        const RayPrep r = ray_prepare(c.r, c.words);
        const int4 v = q.tri[bt];
        if (!tri_hit(r, q.pos[v.x], q.pos[v.y], q.pos[v.z], bd, bp)) bt = kRayNone;
    }
    cast_store_result(t, io, i, c, bt, bd, bp);
}

}  // namespace

void query_decode_sphere(const uint32_t words[kSphereWords], double centre[3], double* radius) {
    sphere_centre(words, centre);
    *radius = sphere_radius(words);
}

void query_launch_sphere(hipStream_t s, const QueryDev& q) {
    if (q.nvis == 0) return;
    (void)hipMemsetAsync(q.sphere, 0, kSphereWords * sizeof(uint32_t), s);
    const uint32_t blocks = std::min((q.nvis + 255u) / 256u, 256u);
    hipLaunchKernelGGL(sphere_minmax_kernel, dim3(blocks), dim3(256), 0, s, q.pos, q.nvis, q.sphere);
    hipLaunchKernelGGL(sphere_radius_kernel, dim3(blocks), dim3(256), 0, s, q.pos, q.nvis, q.sphere);
}

// Few rays: many blocks per ray (one pick must not run on one compute unit); many rays: the rays themselves fill the chip.
uint32_t query_blocks_per_ray(uint32_t ntri, uint32_t count) {
    const uint32_t all = std::max((ntri + 255u) / 256u, 1u), want = std::max(2048u / std::max(count, 1u), 1u);
    return std::min(std::min(all, want), 256u);
}

void query_launch_rays(hipStream_t s, const QueryDev& q, const RayIn* rays, RayPrep* prep, RayCand* cand, RayOut* hits, uint32_t count, uint32_t per_ray) {
    // gridDim.y <= 65535, and a dispatch holds at most 2^32 - 1 work-items (max_grid_blocks)
    const uint32_t chunk = std::min(65535u, max_grid_blocks(256u) / per_ray);
    for (uint32_t first = 0; first < count; first += chunk) {
        const uint32_t n = std::min(chunk, count - first);
        hipLaunchKernelGGL(ray_prep_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, rays + first, n, q.sphere, prep + first);
        hipLaunchKernelGGL(ray_triangles_kernel, dim3(per_ray, n), dim3(256), 0, s, q, prep + first, cand + static_cast<size_t>(first) * per_ray);
        hipLaunchKernelGGL(ray_pick_kernel, dim3((n + 3u) / 4u), dim3(256), 0, s, q, prep + first, cand + static_cast<size_t>(first) * per_ray, per_ray, n, hits + first);
    }
}

void query_launch_body_spheres(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b) {
    (void)hipMemsetAsync(b.spheres, 0, static_cast<size_t>(b.bodies) * kSphereWords * sizeof(uint32_t), s);
    if (q.nvis == 0) return;
    const uint32_t blocks = (q.nvis + 255u) / 256u;   // (<= 2^24: within a dispatch's 2^32 - 1 work-items)
    hipLaunchKernelGGL(body_sphere_minmax_kernel, dim3(blocks), dim3(256), 0, s, q.pos, b.row_body, q.nvis, b.spheres);
    hipLaunchKernelGGL(body_sphere_radius_kernel, dim3(blocks), dim3(256), 0, s, q.pos, b.row_body, q.nvis, b.spheres);
}

void query_launch_spheres_out(hipStream_t s, const QueryBodiesDev& b, char* dst, uint64_t stride) {
    hipLaunchKernelGGL(body_spheres_out_kernel, dim3((b.bodies + 255u) / 256u), dim3(256), 0, s, b.spheres, b.body_rows, b.bodies, dst, stride);
}

// Many rays: the rays themselves fill the chip (one part, the record written by the cast).  Few rays: about four workgroups per compute
// unit's worth of parts, as far as the largest body has tiles and the candidates fit their buffer.
uint32_t query_cast_splits(uint32_t tiles, uint32_t count) {
    const uint32_t groups = (count + kCastTile - 1u) / kCastTile;
    const uint32_t want = std::max(1024u / std::max(groups, 1u), 1u), fit = std::max(kCastCandCap / std::max(count, 1u), 1u);
    return std::min(std::min(std::max(tiles, 1u), std::min(want, fit)), 65535u);
}

void query_launch_cast_device(hipStream_t s, const QueryDev& q, const QueryBodiesDev& b, const CastIo& io, RayCand* cand) {
    const uint32_t tiles = io.body ? b.max_tiles : (q.ntri + kCastTile - 1u) / kCastTile;
    const uint32_t parts = query_cast_splits(tiles, io.count);
    if (parts > 1u) {   // (parts * count <= kCastCandCap: one launch holds every ray)
        hipLaunchKernelGGL(cast_device_kernel<true>, dim3((io.count + kCastTile - 1u) / kCastTile, parts), dim3(256), 0, s, q, b, io, 0u, cand);
        hipLaunchKernelGGL(cast_finish_kernel, dim3((io.count + 255u) / 256u), dim3(256), 0, s, q, b, io, cand, parts);
        return;
    }
    // a dispatch holds at most 2^32 - 1 work-items (max_grid_blocks)
    const uint64_t chunk = static_cast<uint64_t>(max_grid_blocks(256u)) * kCastTile;
    for (uint64_t first = 0; first < io.count; first += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, io.count - first);
        hipLaunchKernelGGL(cast_device_kernel<false>, dim3(static_cast<uint32_t>((n + kCastTile - 1u) / kCastTile)), dim3(256), 0, s, q, b, io, static_cast<uint32_t>(first), cand);
    }
}

}  // namespace tetsim
