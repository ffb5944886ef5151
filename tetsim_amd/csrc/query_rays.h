// query_rays.h -- the device functions the query kernels share (query_kernels.hip: brute force; query_bvh.hip and query_closest.hip: the
// refitted tree): the sphere keys, three.js r160's ray preparation and triangle test, the lexicographic winner, a record's body, and a
// caller's ray and hit records in device memory.  One text for all three units, so that "the existing device function unchanged"
// (include/tetsim.h) holds by construction; all three are built with -ffp-contract=off.  f64 arithmetic on the f32 positions, every
// operation rounded separately, sums left to right.
#pragma once
#include "dev_common.h"
#include "query_device.h"

#include <cmath>
#include <cstring>

namespace tetsim {

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

// the radius from the keys' last two words: the square root of the largest squared distance to the centre (Sphere.radius = sqrt(maxRadiusSq))
__host__ __device__ inline double sphere_radius(const uint32_t* w) {
    double r2;
#if defined(__HIP_DEVICE_COMPILE__)
    r2 = __longlong_as_double(static_cast<long long>(*reinterpret_cast<const unsigned long long*>(w + 6)));
#else
    std::memcpy(&r2, w + 6, 8);
#endif
    return sqrt(r2);
}

// a box grown by a point: the exact f32 min / max (the refit's leaves, a triangle's own box in both traversals)
__device__ inline void box_add(float lo[3], float hi[3], const float4 p) {
    const float v[3] = {p.x, p.y, p.z};
    for (int k = 0; k < 3; k++) { lo[k] = v[k] < lo[k] ? v[k] : lo[k]; hi[k] = v[k] > hi[k] ? v[k] : hi[k]; }
}

__device__ inline double dot3(const double* u, const double* v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }

// Mesh.raycast up to the triangles: the bounding-sphere cull (ray recast by `near`, direction as given), then the ray in the
// mesh's local space -- the identity leaves the origin alone and Vector3.transformDirection normalises the direction.
__device__ inline RayPrep ray_prepare(const RayIn& r, const uint32_t* __restrict__ words) {
    double c[3];
    sphere_centre(words, c);
    const double radius = sphere_radius(words);
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
    return p;
}

// Ray.intersectTriangle(a, b, c, backfaceCulling = true) + checkIntersection's distance window.  true: dist / pt are the hit.
// The triangle's own part (a, e1 = b - a, e2 = c - a, n = e1 x e2) is the same for every ray: TriRec holds it, so that a kernel whose
// rays share a triangle prepares it once.
struct TriRec { double a[3], e1[3], e2[3], n[3]; };
__device__ inline void tri_prepare(const float4 A, const float4 B, const float4 C, TriRec& t) {
    t.a[0] = static_cast<double>(A.x); t.a[1] = static_cast<double>(A.y); t.a[2] = static_cast<double>(A.z);
    t.e1[0] = static_cast<double>(B.x) - t.a[0]; t.e1[1] = static_cast<double>(B.y) - t.a[1]; t.e1[2] = static_cast<double>(B.z) - t.a[2];
    t.e2[0] = static_cast<double>(C.x) - t.a[0]; t.e2[1] = static_cast<double>(C.y) - t.a[1]; t.e2[2] = static_cast<double>(C.z) - t.a[2];
    t.n[0] = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1]; t.n[1] = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2]; t.n[2] = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
}
__device__ inline bool tri_test(const RayPrep& r, const double a[3], const double e1[3], const double e2[3], const double n[3], double& dist, double pt[3]) {
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
__device__ inline bool tri_hit(const RayPrep& r, const float4 A, const float4 B, const float4 C, double& dist, double pt[3]) {
    TriRec t;
    tri_prepare(A, B, C, t);
    return tri_test(r, t.a, t.e1, t.e2, t.n, dist, pt);
}

__device__ inline bool better(double d, uint32_t t, double bd, uint32_t bt) { return t != kRayNone && (bt == kRayNone || d < bd || (d == bd && t < bt)); }

// The body of record i and that body's sphere keys; without a body array, body 0 and the whole mesh's keys.  true: the body is outside the handle.
__device__ inline bool record_body(const QueryDev& q, const QueryBodiesDev& t, const int32_t* body_of, uint32_t i, uint32_t* body, const uint32_t** words) {
    *body = 0u;
    *words = q.sphere;
    if (!body_of) return false;
    const int32_t b = body_of[i];
    if (b < 0 || static_cast<uint32_t>(b) >= t.bodies) return true;
    *body = static_cast<uint32_t>(b);
    *words = t.spheres + static_cast<size_t>(b) * kSphereWords;
    return false;
}

// A caller's ray: its record, what is wrong with it (ray_defect; a body outside the handle), its body and that body's sphere keys.
struct CastRay { RayIn r; uint32_t body; bool bad; const uint32_t* words; };
__device__ inline CastRay cast_load(const QueryDev& q, const QueryBodiesDev& t, const CastIo& io, uint32_t i) {
    CastRay c;
    const double* const src = reinterpret_cast<const double*>(io.in + static_cast<uint64_t>(i) * io.in_stride);
    for (int k = 0; k < 3; k++) { c.r.o[k] = src[k]; c.r.d[k] = src[3 + k]; }
    c.r.near = src[6]; c.r.far = src[7];
    c.bad = ray_defect(c.r.o, c.r.d, c.r.near, c.r.far) != kRayGood;
    if (record_body(q, t, io.body, i, &c.body, &c.words)) c.bad = true;
    return c;
}
// the 48 bytes of a hit record as six 8-byte stores (the record is 8-byte aligned, no more)
__device__ inline void cast_store(const CastIo& io, uint32_t i, int32_t hit, int32_t body, int32_t triangle, double distance, const double pt[3]) {
    unsigned long long* const o = reinterpret_cast<unsigned long long*>(io.out + static_cast<uint64_t>(i) * io.out_stride);
    o[0] = static_cast<unsigned long long>(static_cast<uint32_t>(hit)) | (static_cast<unsigned long long>(static_cast<uint32_t>(body)) << 32);
    o[1] = static_cast<unsigned long long>(static_cast<uint32_t>(triangle));
    o[2] = static_cast<unsigned long long>(__double_as_longlong(distance));
    for (int k = 0; k < 3; k++) o[3 + k] = static_cast<unsigned long long>(__double_as_longlong(pt[k]));
}
__device__ inline void cast_store_result(const QueryBodiesDev& t, const CastIo& io, uint32_t i, const CastRay& c, uint32_t bt, double bd, const double bp[3]) {
    const double zero[3] = {0.0, 0.0, 0.0};
    if (c.bad) cast_store(io, i, -1, -1, -1, 0.0, zero);                  // TETSIM_RAY_INVALID
    else if (bt == kRayNone) cast_store(io, i, 0, -1, -1, 0.0, zero);
    else cast_store(io, i, 1, io.body ? static_cast<int32_t>(c.body) : t.tri_body ? t.tri_body[bt] : 0, static_cast<int32_t>(bt), bd, bp);
}

}  // namespace tetsim
