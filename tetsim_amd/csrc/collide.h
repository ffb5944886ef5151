// collide.h -- kinematic colliders (tetsim_set_colliders, include/tetsim.h): one particle against the call's list, ONE routine per
// arithmetic, inlined into every particle pass (pj_kernels.inc, pjb_vertex_update in pj_blocked.hip, pjq_vertex_update in pj_quad.hip,
// post_vertex in nh_kernels.inc).  They run after the clamp, floor and grab, before the velocity; the caller skips grabbed particles
// and calls them only when DevParams::n_colliders != 0 or DevParams::body_colliders != 0 (a uniform scalar test: a body without colliders
// runs its old code).  The routines walk a list (dt, entries, count); where the list comes from is the caller's business -- the handle's
// list in DevParams (uniform addresses: scalar loads) or, with body colliders on (tetsim_set_body_colliders), the entries of the
// particle's body in the table (dev_common.h: body_colliders_pick), made uniform wave by wave -- collide_particle_* below.
//
// The definition (tetsim.h restates it), p = position so far, q = end of the previous substep, dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z:
//   sphere   d = p - a, L = sqrt(dot(d, d)); hit = L < r && L > 0; n = d / L, depth = r - L
//   capsule  ab = b - a, t = dot(p - a, ab) / dot(ab, ab) (0 if dot(ab, ab) == 0), t = min(max(t, 0), 1); d = p - (a + ab*t), as the sphere
//   box      l_k = dot(p - a, u_k); hit iff |l_k| < e_k for all k; k = argmin e_k - |l_k| (lowest on ties); n = l_k >= 0 ? u_k : -u_k
//   plane    s = dot(p - a, n); hit = s < 0, depth = -s
//   response p = p + n*depth; D = (q - p) + V*dt; T = D - n*dot(D, n); p = p + T*min(1, dt*friction)
// f32 (collide_f32<kFast>): PRECISE is the order above with separate roundings (its unit is built with -ffp-contract=off) and correctly
// rounded / and sqrt; FAST spells every multiply-add out as fmaf and divides through v_rcp -- no product is left for the backend to fuse,
// so every call site of a unit rounds alike (pjb_vertex_update's call sites must agree bit for bit).  f64 (collide_f64): Softbody.js's
// arithmetic -- f64 on the stored f32 values, Math.min / Math.max, p stored (rounded to f32) after the push and after the friction.
#pragma once
#include "dev_common.h"

namespace tetsim {
namespace collide {

template <bool kFast> __device__ __forceinline__ float mad(float a, float b, float c) {
    if constexpr (kFast) return __builtin_fmaf(a, b, c);
    else return a * b + c;
}
template <bool kFast> __device__ __forceinline__ float dot(float ax, float ay, float az, float bx, float by, float bz) {
    if constexpr (kFast) return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
    else return (ax * bx + ay * by) + az * bz;
}
template <bool kFast> __device__ __forceinline__ float div(float a, float b, float rb) {
    if constexpr (kFast) return a * rb;
    else return a / b;
}
template <bool kFast> __device__ __forceinline__ float rcp(float b) {
    if constexpr (kFast) return __builtin_amdgcn_rcpf(b);
    else return b;   // (unused: PRECISE divides)
}

// Math.max / Math.min of JS numbers (NaN-propagating, -0 < +0), as nh_kernels.inc
__device__ __forceinline__ double js_max(double a, double b) {
    if (a != a || b != b) return a + b;
    if (a == 0.0 && b == 0.0) return __builtin_signbit(a) ? b : a;
    return a > b ? a : b;
}
__device__ __forceinline__ double js_min(double a, double b) {
    if (a != a || b != b) return a + b;
    if (a == 0.0 && b == 0.0) return __builtin_signbit(a) ? a : b;
    return a < b ? a : b;
}

}  // namespace collide

// One particle (px, py, pz) against the `count` colliders of `col`, in list order; (qx, qy, qz) = end of the previous substep.  f32 view.
template <bool kFast>
__device__ __forceinline__ void collide_f32(float& px, float& py, float& pz, const float qx, const float qy, const float qz, const float dt,
                                            const DevColliderF* col, const uint32_t count) {
    using namespace collide;
    for (uint32_t k = 0; k < count; k++) {
        const DevColliderF& C = col[k];
        bool hit = false;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, depth = 0.0f;
        if (C.kind == 0 || C.kind == 1) {   // sphere, capsule: the distance to a point (the centre, the nearest point of the segment)
            float cx = C.a[0], cy = C.a[1], cz = C.a[2];
            if (C.kind == 1) {
                const float abx = C.b[0] - C.a[0], aby = C.b[1] - C.a[1], abz = C.b[2] - C.a[2];
                const float ab2 = dot<kFast>(abx, aby, abz, abx, aby, abz);
                float t = 0.0f;
                if (ab2 != 0.0f) {
                    const float num = dot<kFast>(px - C.a[0], py - C.a[1], pz - C.a[2], abx, aby, abz);
                    t = div<kFast>(num, ab2, rcp<kFast>(ab2));
                    // FAST: num * rcp(ab2) can fall an ulp short of 1 where num >= ab2 -- a particle exactly on b then stood an ulp off the
                    // nearest point, L > 0, and was thrown out by r along rounding noise.  t >= 1 iff num >= ab2: decide it there.
                    if constexpr (kFast) { if (num >= ab2) t = 1.0f; }
                }
                t = fminf(fmaxf(t, 0.0f), 1.0f);
                cx = mad<kFast>(abx, t, C.a[0]); cy = mad<kFast>(aby, t, C.a[1]); cz = mad<kFast>(abz, t, C.a[2]);
            }
            const float dx = px - cx, dy = py - cy, dz = pz - cz;
            const float L = __builtin_sqrtf(dot<kFast>(dx, dy, dz, dx, dy, dz));
            hit = L < C.radius && L > 0.0f;
            if (hit) {
                const float rL = rcp<kFast>(L);
                nx = div<kFast>(dx, L, rL); ny = div<kFast>(dy, L, rL); nz = div<kFast>(dz, L, rL);
                depth = C.radius - L;
            }
        } else if (C.kind == 2) {   // box
            const float dx = px - C.a[0], dy = py - C.a[1], dz = pz - C.a[2];
            float l[3], g[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                l[j] = dot<kFast>(dx, dy, dz, C.u[3 * j], C.u[3 * j + 1], C.u[3 * j + 2]);
                g[j] = C.b[j] - fabsf(l[j]);
            }
            hit = fabsf(l[0]) < C.b[0] && fabsf(l[1]) < C.b[1] && fabsf(l[2]) < C.b[2];
            if (hit) {
                int j = 0;
                if (g[1] < g[j]) j = 1;
                if (g[2] < g[j]) j = 2;
                const float sgn = l[j] >= 0.0f ? 1.0f : -1.0f;
                nx = sgn * C.u[3 * j]; ny = sgn * C.u[3 * j + 1]; nz = sgn * C.u[3 * j + 2];
                depth = g[j];
            }
        } else {   // plane
            nx = C.b[0]; ny = C.b[1]; nz = C.b[2];
            const float s = dot<kFast>(px - C.a[0], py - C.a[1], pz - C.a[2], nx, ny, nz);
            hit = s < 0.0f;
            depth = -s;
        }
        if (!hit) continue;
        px = mad<kFast>(nx, depth, px); py = mad<kFast>(ny, depth, py); pz = mad<kFast>(nz, depth, pz);
        const float Dx = mad<kFast>(C.v[0], dt, qx - px), Dy = mad<kFast>(C.v[1], dt, qy - py), Dz = mad<kFast>(C.v[2], dt, qz - pz);
        const float dn = dot<kFast>(Dx, Dy, Dz, nx, ny, nz);
        float Tx, Ty, Tz;
        if constexpr (kFast) { Tx = __builtin_fmaf(-nx, dn, Dx); Ty = __builtin_fmaf(-ny, dn, Dy); Tz = __builtin_fmaf(-nz, dn, Dz); }
        else { Tx = Dx - nx * dn; Ty = Dy - ny * dn; Tz = Dz - nz * dn; }
        const float m = fminf(1.0f, dt * C.friction);
        px = mad<kFast>(Tx, m, px); py = mad<kFast>(Ty, m, py); pz = mad<kFast>(Tz, m, pz);
    }
}

// ... against the handle's list (the form every call site had before there were two kinds of list: the same text, the same bits)
template <bool kFast>
__device__ __forceinline__ void collide_f32(float& px, float& py, float& pz, const float qx, const float qy, const float qz, const DevParams& P) {
    collide_f32<kFast>(px, py, pz, qx, qy, qz, P.dt, P.col, P.n_colliders);
}

// The same in Softbody.js's arithmetic (PRECISE Neo-Hookean): f64 view of the colliders, f64 dt, f32 stores.
__device__ __forceinline__ void collide_f64(float& px, float& py, float& pz, const float qx, const float qy, const float qz, const double dt,
                                            const DevColliderD* col, const uint32_t count) {
    using collide::js_max;
    using collide::js_min;
    for (uint32_t k = 0; k < count; k++) {
        const DevColliderD& C = col[k];
        const double x = px, y = py, z = pz;
        bool hit = false;
        double nx = 0.0, ny = 0.0, nz = 0.0, depth = 0.0;
        if (C.kind == 0 || C.kind == 1) {
            double cx = C.a[0], cy = C.a[1], cz = C.a[2];
            if (C.kind == 1) {
                const double abx = C.b[0] - C.a[0], aby = C.b[1] - C.a[1], abz = C.b[2] - C.a[2];
                const double ab2 = (abx * abx + aby * aby) + abz * abz;
                double t = 0.0;
                if (ab2 != 0.0) t = (((x - C.a[0]) * abx + (y - C.a[1]) * aby) + (z - C.a[2]) * abz) / ab2;
                t = js_min(js_max(t, 0.0), 1.0);
                cx = C.a[0] + abx * t; cy = C.a[1] + aby * t; cz = C.a[2] + abz * t;
            }
            const double dx = x - cx, dy = y - cy, dz = z - cz;
            const double L = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
            hit = L < C.radius && L > 0.0;
            if (hit) { nx = dx / L; ny = dy / L; nz = dz / L; depth = C.radius - L; }
        } else if (C.kind == 2) {
            const double dx = x - C.a[0], dy = y - C.a[1], dz = z - C.a[2];
            double l[3], g[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                l[j] = (dx * C.u[3 * j] + dy * C.u[3 * j + 1]) + dz * C.u[3 * j + 2];
                g[j] = C.b[j] - __builtin_fabs(l[j]);
            }
            hit = __builtin_fabs(l[0]) < C.b[0] && __builtin_fabs(l[1]) < C.b[1] && __builtin_fabs(l[2]) < C.b[2];
            if (hit) {
                int j = 0;
                if (g[1] < g[j]) j = 1;
                if (g[2] < g[j]) j = 2;
                const double sgn = l[j] >= 0.0 ? 1.0 : -1.0;
                nx = sgn * C.u[3 * j]; ny = sgn * C.u[3 * j + 1]; nz = sgn * C.u[3 * j + 2];
                depth = g[j];
            }
        } else {
            nx = C.b[0]; ny = C.b[1]; nz = C.b[2];
            const double s = ((x - C.a[0]) * nx + (y - C.a[1]) * ny) + (z - C.a[2]) * nz;
            hit = s < 0.0;
            depth = -s;
        }
        if (!hit) continue;
        px = static_cast<float>(x + nx * depth); py = static_cast<float>(y + ny * depth); pz = static_cast<float>(z + nz * depth);
        const double Dx = (static_cast<double>(qx) - static_cast<double>(px)) + C.v[0] * dt;
        const double Dy = (static_cast<double>(qy) - static_cast<double>(py)) + C.v[1] * dt;
        const double Dz = (static_cast<double>(qz) - static_cast<double>(pz)) + C.v[2] * dt;
        const double dn = (Dx * nx + Dy * ny) + Dz * nz;
        const double m = js_min(1.0, dt * C.friction);
        px = static_cast<float>(static_cast<double>(px) + (Dx - nx * dn) * m);
        py = static_cast<float>(static_cast<double>(py) + (Dy - ny * dn) * m);
        pz = static_cast<float>(static_cast<double>(pz) + (Dz - nz * dn) * m);
    }
}
__device__ __forceinline__ void collide_f64(float& px, float& py, float& pz, const float qx, const float qy, const float qz, const DevParams& P) {
    collide_f64(px, py, pz, qx, qy, qz, P.d_dt, P.d_col, P.n_colliders);
}

// The uniform test of every call site, and what stands behind it.  A wave may hold particles of several bodies (the particle kernels' blocks
// span bodies): the lanes that have a particle to push (`push`: not held) are served body by body -- the first waiting lane's body index
// becomes a uniform value, the lanes of that body walk its list, read with scalar loads, and leave; one trip while body colliders are off
// (every lane says body 0, the list is the handle's) and wherever a wave holds one body.  No arithmetic of its own.
__device__ __forceinline__ bool any_colliders(const DevParams& P) { return (P.n_colliders | P.body_colliders) != 0u; }
template <bool kFast>
__device__ __forceinline__ void collide_particle_f32(float& px, float& py, float& pz, const float qx, const float qy, const float qz, const DevParams& P, const uint32_t v, bool push) {
    const uint32_t body = body_colliders_body(P, v);
    while (push) {
        const uint32_t now = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int32_t>(body)));
        if (body == now) {
            const DevColliderF* list;
            uint32_t count;
            body_colliders_pick(P, now, &list, &count);
            collide_f32<kFast>(px, py, pz, qx, qy, qz, P.dt, list, count);
            push = false;
        }
    }
}
__device__ __forceinline__ void collide_particle_f64(float& px, float& py, float& pz, const float qx, const float qy, const float qz, const DevParams& P, const uint32_t v, bool push) {
    const uint32_t body = body_colliders_body(P, v);
    while (push) {
        const uint32_t now = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int32_t>(body)));
        if (body == now) {
            const DevColliderD* list;
            uint32_t count;
            body_colliders_pick(P, now, &list, &count);
            collide_f64(px, py, pz, qx, qy, qz, P.d_dt, list, count);
            push = false;
        }
    }
}

}  // namespace tetsim
