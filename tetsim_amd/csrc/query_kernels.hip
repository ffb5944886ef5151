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

#include <algorithm>
#include <cmath>
#include <cstring>

namespace tetsim {
namespace {

// f32 -> u32 with the same order (negative values: all bits flipped; others: the top bit set), and back
__host__ __device__ inline uint32_t key_of(uint32_t bits) { return (bits >> 31) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ inline uint32_t bits_of(uint32_t key) { return (key >> 31) ? (key & 0x7fffffffu) : ~key; }

__host__ __device__ inline void sphere_centre(const uint32_t* w, double c[3]) {
    for (int k = 0; k < 3; k++) {
        const uint32_t lo = bits_of(~w[k]), hi = bits_of(w[3 + k]);
        float flo, fhi;
#if defined(__HIP_DEVICE_COMPILE__)
        flo = __uint_as_float(lo); fhi = __uint_as_float(hi);
#else
        std::memcpy(&flo, &lo, 4); std::memcpy(&fhi, &hi, 4);
#endif
        c[k] = (static_cast<double>(flo) + static_cast<double>(fhi)) * 0.5;   // Box3.getCenter: addVectors(min, max).multiplyScalar(0.5)
    }
}

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

__device__ inline double dot3(const double* u, const double* v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }

// Mesh.raycast up to the triangles: the bounding-sphere cull (ray recast by `near`, direction as given), then the ray in the
// mesh's local space -- the identity leaves the origin alone and Vector3.transformDirection normalises the direction.
__global__ __launch_bounds__(256) void ray_prep_kernel(const RayIn* __restrict__ rays, uint32_t count, const uint32_t* __restrict__ words, RayPrep* __restrict__ prep) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const RayIn r = rays[i];
    double c[3];
    sphere_centre(words, c);
    const double radius = sqrt(__longlong_as_double(static_cast<long long>(*reinterpret_cast<const unsigned long long*>(words + 6))));
    const double radius2 = radius * radius;
    double o2[3], v[3];
    for (int k = 0; k < 3; k++) o2[k] = r.o[k] + r.d[k] * r.near;          // Ray.recast(near) = at(near)
    for (int k = 0; k < 3; k++) v[k] = o2[k] - c[k];
    bool culled = false;
    if (!(dot3(v, v) <= radius2)) {                                          // Sphere.containsPoint(origin) === false
        for (int k = 0; k < 3; k++) v[k] = c[k] - o2[k];                     // Ray.intersectSphere
        const double tca = dot3(v, r.d);
        const double d2 = dot3(v, v) - tca * tca;
        if (d2 > radius2) culled = true;
        else {
            const double thc = sqrt(radius2 - d2);
            const double t0 = tca - thc, t1 = tca + thc;
            if (t1 < 0.0) culled = true;
            else {
                const double t = t0 < 0.0 ? t1 : t0;
                double w[3];
                for (int k = 0; k < 3; k++) w[k] = o2[k] - (o2[k] + r.d[k] * t);   // origin.distanceToSquared(at(t))
                const double span = r.far - r.near;
                if (dot3(w, w) > span * span) culled = true;
            }
        }
    }
    double len = sqrt(r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2]);   // normalize(): divideScalar(length() || 1) = multiplyScalar(1 / s)
    if (len == 0.0 || len != len) len = 1.0;
    const double s = 1.0 / len;
    RayPrep p;
    for (int k = 0; k < 3; k++) { p.o[k] = r.o[k]; p.d[k] = r.d[k] * s; }
    p.near = r.near; p.far = r.far; p.culled = culled ? 1u : 0u; p.pad = 0u;
    prep[i] = p;
}

// Ray.intersectTriangle(a, b, c, backfaceCulling = true) + checkIntersection's distance window.  true: dist / pt are the hit.
__device__ inline bool tri_hit(const RayPrep& r, const float4 A, const float4 B, const float4 C, double& dist, double pt[3]) {
    const double a[3] = {static_cast<double>(A.x), static_cast<double>(A.y), static_cast<double>(A.z)};
    const double e1[3] = {static_cast<double>(B.x) - a[0], static_cast<double>(B.y) - a[1], static_cast<double>(B.z) - a[2]};
    const double e2[3] = {static_cast<double>(C.x) - a[0], static_cast<double>(C.y) - a[1], static_cast<double>(C.z) - a[2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    double DdN = dot3(r.d, n);
    if (!(DdN < 0.0)) return false;          // > 0: a back face, culled (front-side material); == 0 (or NaN): no intersection
    DdN = -DdN;                              // sign = -1
    const double diff[3] = {r.o[0] - a[0], r.o[1] - a[1], r.o[2] - a[2]};
    const double qxe2[3] = {diff[1] * e2[2] - diff[2] * e2[1], diff[2] * e2[0] - diff[0] * e2[2], diff[0] * e2[1] - diff[1] * e2[0]};
    const double DdQxE2 = -dot3(r.d, qxe2);
    if (DdQxE2 < 0.0) return false;
    const double e1xq[3] = {e1[1] * diff[2] - e1[2] * diff[1], e1[2] * diff[0] - e1[0] * diff[2], e1[0] * diff[1] - e1[1] * diff[0]};
    const double DdE1xQ = -dot3(r.d, e1xq);
    if (DdE1xQ < 0.0) return false;
    if (DdQxE2 + DdE1xQ > DdN) return false;
    const double QdN = dot3(diff, n);        // -sign * diff.n
    if (QdN < 0.0) return false;
    const double t = QdN / DdN;
    double w[3];
    for (int k = 0; k < 3; k++) { pt[k] = r.o[k] + r.d[k] * t; w[k] = r.o[k] - pt[k]; }   // Ray.at; origin.distanceTo(point)
    dist = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    return !(dist < r.near || dist > r.far);
}

__device__ inline bool better(double d, uint32_t t, double bd, uint32_t bt) { return t != kRayNone && (bt == kRayNone || d < bd || (d == bd && t < bt)); }

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

}  // namespace

void query_decode_sphere(const uint32_t words[kSphereWords], double centre[3], double* radius) {
    sphere_centre(words, centre);
    double r2;
    std::memcpy(&r2, words + 6, 8);
    *radius = std::sqrt(r2);
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

}  // namespace tetsim
