// nh_kernels.inc -- NEOHOOKEAN_GS substep kernels for gfx950, included by nh_precise.hip (T = double,
// -ffp-contract=off) and nh_fast.hip (T = float).
//
// The reference CPU solver (Softbody.js:91-240) computes in f64 and rounds to f32 at every
// Float32Array store.  The PRECISE build does exactly that on the device -- same operations, same order,
// same rounding points, no FMA fusion -- so its trajectories are bit-identical to the reference's
// (MI355X runs f64 vector math at half the f32 rate, and this kernel is gather/latency bound anyway).
//
// Gauss-Seidel is made parallel without changing its result: tets are processed level by level
// (host_prep.cpp prep_levels); tets of one level share no vertex, and any two tets that do share a
// vertex keep their sequential order, so every lane sees exactly the positions the sequential sweep
// would have given it.
#include "collide.h"
#include "dev_common.h"
#include "dev_store.h"

// kernels and launchers carry the arithmetic mode in their names (pj_tet_kernel_precise / _fast ...)
#define TETSIM_CAT_(a, b) a##b
#define TETSIM_CAT(a, b) TETSIM_CAT_(a, b)
#define TETSIM_SFX(name) TETSIM_CAT(name, TETSIM_MODE_SUFFIX)

namespace tetsim {
namespace {

#if TETSIM_FAST
// FAST fuses a * b + c into one operation only where it is WRITTEN as one expression (the unit is built with -ffp-contract=on,
// tetsim_amd/build.py): what several kernels share (solve_elem, solve_quad, predict_vertex, post_vertex) then rounds the same way
// wherever it is inlined, and a body's stepwise kernels agree with its fused ones bit for bit by construction.  (With
// -ffp-contract=fast the BACKEND fuses any multiply with any add, pragma or not, and which pairs it picks depends on the code
// around them: the single-workgroup launch of small bodies and its stepwise twin disagreed in one tet out of a few hundred.
// Nothing lost: the four-lane cluster kernel measures 63.5-64.7 us per substep on the 1 M-tet lattice this way, 65.5 before.)
#pragma clang fp contract(on)
using T = float;
#else
using T = double;
#endif

__device__ __forceinline__ float fr(T x) { return static_cast<float>(x); }
__device__ __forceinline__ T sqrt_(T x) {
#if TETSIM_FAST
    return sqrtf(x);
#else
    return sqrt(x);  // correctly rounded, like Math.sqrt
#endif
}

struct g3 { float x, y, z; };  // an f32-stored 3-vector (one row of a Float32Array)

// a += b*scale with the store rounding of vecAdd (Softbody.js:316-321)
__device__ __forceinline__ void vec_add(g3& a, const g3& b, T scale) {
    a.x = fr(static_cast<T>(a.x) + static_cast<T>(b.x) * scale);
    a.y = fr(static_cast<T>(a.y) + static_cast<T>(b.y) * scale);
    a.z = fr(static_cast<T>(a.z) + static_cast<T>(b.z) * scale);
}
// vecSetDiff with scale 1.0 (Softbody.js:323-328); (a-b)*1.0 == a-b exactly
__device__ __forceinline__ g3 vec_diff(const g3& a, const g3& b) {
    g3 r;
    r.x = fr(static_cast<T>(a.x) - static_cast<T>(b.x));
    r.y = fr(static_cast<T>(a.y) - static_cast<T>(b.y));
    r.z = fr(static_cast<T>(a.z) - static_cast<T>(b.z));
    return r;
}
__device__ __forceinline__ T len2(const g3& a) {  // vecLengthSquared :330-334
    const T a0 = a.x, a1 = a.y, a2 = a.z;
    return a0 * a0 + a1 * a1 + a2 * a2;
}
__device__ __forceinline__ g3 cross_store(const g3& b, const g3& c) {  // vecSetCross :343-348
    const T b0 = b.x, b1 = b.y, b2 = b.z, c0 = c.x, c1 = c.y, c2 = c.z;
    g3 r;
    r.x = fr(b1 * c2 - b2 * c1);
    r.y = fr(b2 * c0 - b0 * c2);
    r.z = fr(b0 * c1 - b1 * c0);
    return r;
}
__device__ __forceinline__ g3 zero3() { g3 r; r.x = 0.0f; r.y = 0.0f; r.z = 0.0f; return r; }

// F = P * invRestPose (matSetMatProduct :374-379): column j = ((0 + P0*b0) + P1*b1) + P2*b2
__device__ __forceinline__ void f_from_p(g3 F[3], const g3 P[3], const float ir[9]) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
        F[j] = zero3();
        vec_add(F[j], P[0], static_cast<T>(ir[3 * j + 0]));
        vec_add(F[j], P[1], static_cast<T>(ir[3 * j + 1]));
        vec_add(F[j], P[2], static_cast<T>(ir[3 * j + 2]));
    }
}

// applyToElem, Softbody.js:168-193.  g[1..3] in, positions updated in registers.
__device__ __forceinline__ void apply_to_elem(g3 p[4], const float im[4], g3 g[4], T C, T alpha) {
    if (C == static_cast<T>(0)) return;
    g[0] = zero3();
    vec_add(g[0], g[1], static_cast<T>(-1.0));
    vec_add(g[0], g[2], static_cast<T>(-1.0));
    vec_add(g[0], g[3], static_cast<T>(-1.0));
    T w = static_cast<T>(0);
#pragma unroll
    for (int i = 0; i < 4; i++) w += len2(g[i]) * static_cast<T>(im[i]);
    if (w == static_cast<T>(0)) return;
#if TETSIM_FAST
    const T dlambda = -C * __builtin_amdgcn_rcpf(w + alpha);
#else
    const T dlambda = -C / (w + alpha);
#endif
#pragma unroll
    for (int i = 0; i < 4; i++) vec_add(p[i], g[i], dlambda * static_cast<T>(im[i]));
}

// solveElem, Softbody.js:91-166, on the four corners in registers; returns det F - 1 (the tet's volError term, :163).
__device__ __forceinline__ T solve_elem(g3 p[4], const float im[4], const float ir[9], T irv, T dt, T devC, T volC) {
    g3 Pm[3], F[3], g[4];
    // ---- deviatoric, C = sqrt(tr(F^T F)) (:103-130)
    Pm[0] = vec_diff(p[1], p[0]); Pm[1] = vec_diff(p[2], p[0]); Pm[2] = vec_diff(p[3], p[0]);
    f_from_p(F, Pm, ir);
#if TETSIM_FAST
    const T r_s2 = len2(F[0]) + len2(F[1]) + len2(F[2]);
    // (a collapsed tet: r_s2 == 0 -> rsq = inf and 0 * inf = NaN, for which `C != 0` holds and NaNs would be written.  Softbody.js
    // returns early there -- sqrt(0) == 0 == C, :176 -- so C is forced to 0: the NaN gradients are then never used.)
    const T r_s_inv = __builtin_amdgcn_rsqf(r_s2);
    const T r_s = r_s2 > static_cast<T>(0) ? r_s2 * r_s_inv : static_cast<T>(0);
#else
    const T r_s = sqrt_(len2(F[0]) + len2(F[1]) + len2(F[2]));
    const T r_s_inv = static_cast<T>(1.0) / r_s;
#endif
#pragma unroll
    for (int k = 0; k < 3; k++) {  // g_{k+1} += F_j * (r_s_inv * ir(row k, col j)),  matIJ :359-361
        g[k + 1] = zero3();
        vec_add(g[k + 1], F[0], r_s_inv * static_cast<T>(ir[3 * 0 + k]));
        vec_add(g[k + 1], F[1], r_s_inv * static_cast<T>(ir[3 * 1 + k]));
        vec_add(g[k + 1], F[2], r_s_inv * static_cast<T>(ir[3 * 2 + k]));
    }
    apply_to_elem(p, im, g, r_s, devC / dt / dt * irv);

    // ---- hydrostatic, C = det F - 1 - volCompliance/devCompliance (:134-165)
    Pm[0] = vec_diff(p[1], p[0]); Pm[1] = vec_diff(p[2], p[0]); Pm[2] = vec_diff(p[3], p[0]);
    f_from_p(F, Pm, ir);
    g3 dF[3];
    dF[0] = cross_store(F[1], F[2]);
    dF[1] = cross_store(F[2], F[0]);
    dF[2] = cross_store(F[0], F[1]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        g[k + 1] = zero3();
        vec_add(g[k + 1], dF[0], static_cast<T>(ir[3 * 0 + k]));
        vec_add(g[k + 1], dF[1], static_cast<T>(ir[3 * 1 + k]));
        vec_add(g[k + 1], dF[2], static_cast<T>(ir[3 * 2 + k]));
    }
    T vol;
    {  // matGetDeterminant(F) :381-387, term order as written
        const T a11 = F[0].x, a12 = F[1].x, a13 = F[2].x;
        const T a21 = F[0].y, a22 = F[1].y, a23 = F[2].y;
        const T a31 = F[0].z, a32 = F[1].z, a33 = F[2].z;
        vol = a11 * a22 * a33 + a12 * a23 * a31 + a13 * a21 * a32 - a13 * a22 * a31 - a12 * a21 * a33 - a11 * a23 * a32;
    }
    const T C = vol - static_cast<T>(1.0) - volC / devC;
    apply_to_elem(p, im, g, C, volC / dt / dt * irv);
    return vol - static_cast<T>(1.0);
}

// Body parameters in a tet solve (tetsim_set_body_params): behind ONE uniform branch the two compliances come from the row of the body of
// tet e (solve position; DevParams::tet_body), in this unit's arithmetic -- only where the values come from, the solve's text is untouched.
__device__ __forceinline__ void body_compliances(const DevParams& P, uint32_t e, T& devC, T& volC) {
    if (P.body_params) {
        const auto* const r = body_params_row(P, P.tet_body[e], T());
        devC = r->dev_compliance; volC = r->vol_compliance;
    }
}
__device__ __forceinline__ uint32_t cluster_body(const DevParams& P, uint32_t e) { return P.body_params ? P.tet_body[e] : 0u; }   // e: any tet of the cluster
// ... with the body index at hand (one workgroup per body: uniform, scalar loads)
__device__ __forceinline__ void body_compliances_of(const DevParams& P, uint32_t body, T& devC, T& volC) {
    if (P.body_params) {
        const auto* const r = body_params_row(P, body, T());
        devC = r->dev_compliance; volC = r->vol_compliance;
    }
}
// What every tet solve starts from, in this unit's arithmetic: the time step and the two compliances of the handle -- of the body of tet e
// where one is named (body_compliances; a cluster's tets and particles are one body's, so its first tet names it).
struct TetScalars { T dt, devC, volC; };
__device__ __forceinline__ TetScalars tet_scalars(const DevParams& P) {
#if TETSIM_FAST
    return {P.dt, static_cast<T>(P.d_dev_compliance), static_cast<T>(P.d_vol_compliance)};
#else
    return {P.d_dt, P.d_dev_compliance, P.d_vol_compliance};
#endif
}
__device__ __forceinline__ TetScalars tet_scalars(const DevParams& P, uint32_t e) {
    TetScalars s = tet_scalars(P);
    body_compliances(P, e, s.devC, s.volC);
    return s;
}
// ... and what solve_quad takes in their place: a_dev = devCompliance / dt / dt, a_vol likewise (left to right, as `devC / dt / dt * irv`
// evaluates in solve_elem), c_off = volCompliance / devCompliance
struct QuadScalars { T a_dev, a_vol, c_off; };
__device__ __forceinline__ QuadScalars quad_scalars(const TetScalars& s) { return {s.devC / s.dt / s.dt, s.volC / s.dt / s.dt, s.volC / s.devC}; }

// One dependency level: lanes [first, first+count) of the solve order.
template <bool kWriteThrough>
__global__ __launch_bounds__(256) void TETSIM_SFX(nh_level_kernel_)(NHDev d, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t e = first + i;
    const TetScalars S = tet_scalars(*d.params, e);
    const int4 id = d.tet_idx[e];
    const float4 ia = d.irp_a[e], ib = d.irp_b[e], ic = d.irp_c[e];
    const float ir[9] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w, ic.x};
    float4 p4[4];
    p4[0] = d.pos[id.x]; p4[1] = d.pos[id.y]; p4[2] = d.pos[id.z]; p4[3] = d.pos[id.w];
    g3 p[4];
    float im[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { p[k].x = p4[k].x; p[k].y = p4[k].y; p[k].z = p4[k].z; im[k] = p4[k].w; }
    const T ve = solve_elem(p, im, ir, static_cast<T>(ic.y), S.dt, S.devC, S.volC);
    if (d.vol_err) d.vol_err[d.order[e]] = static_cast<double>(ve);   // (null in a sweep that is not its call's last: the call leaves its LAST sweep's behind)
    if constexpr (kWriteThrough) {  // big levels: the next level's launch reads these from other CUs and XCDs (see the cluster kernel)
        store_wt(d.pos, static_cast<uint32_t>(id.x), make_float4(p[0].x, p[0].y, p[0].z, im[0]));
        store_wt(d.pos, static_cast<uint32_t>(id.y), make_float4(p[1].x, p[1].y, p[1].z, im[1]));
        store_wt(d.pos, static_cast<uint32_t>(id.z), make_float4(p[2].x, p[2].y, p[2].z, im[2]));
        store_wt(d.pos, static_cast<uint32_t>(id.w), make_float4(p[3].x, p[3].y, p[3].z, im[3]));
    } else {
        d.pos[id.x] = make_float4(p[0].x, p[0].y, p[0].z, im[0]);
        d.pos[id.y] = make_float4(p[1].x, p[1].y, p[1].z, im[1]);
        d.pos[id.z] = make_float4(p[2].x, p[2].y, p[2].z, im[2]);
        d.pos[id.w] = make_float4(p[3].x, p[3].y, p[3].z, im[3]);
    }
}

// The per-particle passes' parameters as VALUES: read once per kernel.  (References into *d.params would be re-read from
// memory after every write-through store -- an asm statement with a memory clobber -- and a vector load behind such a store
// waits for the store's full trip to HBM: 1.2 us per particle in the cluster kernel's write-back loop.)
struct VParams {
    T dt, gravity, friction, lo[3], hi[3];
    int32_t grab_local;
    float grab[3];
    uint32_t body_grabs;           // non-zero: a table's row decides (tetsim_set_body_grabs, tetsim_set_body_pins: dev_common.h), grab_local / grab are not looked at
    const uint32_t* grab_body;     // the table's two addresses as values; post_vertex reads a particle's row before anything is stored
    const int4* grab_rows;
    const DevParams* all;   // the colliders (collide.h)
};
__device__ __forceinline__ VParams load_vparams(const DevParams& P) {
    VParams q;
#if TETSIM_FAST
    q.dt = P.dt; q.gravity = P.gravity; q.friction = P.friction;
#else
    q.dt = P.d_dt; q.gravity = P.d_gravity; q.friction = P.d_friction;
#endif
#pragma unroll
    for (int k = 0; k < 3; k++) { q.lo[k] = static_cast<T>(P.d_lo[k]); q.hi[k] = static_cast<T>(P.d_hi[k]); q.grab[k] = P.grab[k]; }
    q.grab_local = P.grab_local;
    q.body_grabs = P.body_grabs; q.grab_body = P.grab_body; q.grab_rows = P.grab_rows;
    q.all = &P;
    return q;
}
// ... for a particle of `body`: with body parameters on (tetsim_set_body_params), behind one uniform branch, gravity, friction and the
// bounds are those of the body's row
__device__ __forceinline__ VParams load_vparams_of(const DevParams& P, uint32_t body) {
    VParams q = load_vparams(P);
    if (P.body_params) {
        const auto* const r = body_params_row(P, body, T());
        q.gravity = r->gravity; q.friction = r->friction;
#pragma unroll
        for (int k = 0; k < 3; k++) { q.lo[k] = r->lo[k]; q.hi[k] = r->hi[k]; }
    }
    return q;
}
// ... for particle v (device index), whose body the particle -> body array names: a lane of its own, a wave that spans bodies
__device__ __forceinline__ VParams load_vparams(const DevParams& P, uint32_t v) { return load_vparams_of(P, P.body_params ? P.grab_body[v] : 0u); }

// XPBD prediction, Softbody.js:198-202: vel and pos in, (vel, prev, pos) out
__device__ __forceinline__ void predict_vertex(const VParams& P, float4& vel, float4& pos, float4& prev) {
    const T dt = P.dt, g = P.gravity;
#if !TETSIM_FAST   // (FAST: x + 0 * dt is x for every finite dt, up to the sign of a zero)
    vel.x = fr(static_cast<T>(vel.x) + static_cast<T>(0.0) * dt);  // vecAdd(vel, i, [0, gravity, 0], 0, dt)
    vel.z = fr(static_cast<T>(vel.z) + static_cast<T>(0.0) * dt);
#endif
    vel.y = fr(static_cast<T>(vel.y) + g * dt);
    prev = pos;
    pos.x = fr(static_cast<T>(pos.x) + static_cast<T>(vel.x) * dt);
    pos.y = fr(static_cast<T>(pos.y) + static_cast<T>(vel.y) * dt);
    pos.z = fr(static_cast<T>(pos.z) + static_cast<T>(vel.z) * dt);
}
__global__ __launch_bounds__(256) void TETSIM_SFX(nh_predict_kernel_)(NHDev d) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= d.nv) return;
    float4 vel = d.vel[v], pos = d.pos[v], prev;
    predict_vertex(load_vparams(*d.params, v), vel, pos, prev);
    d.vel[v] = vel;
    d.prev[v] = prev;
    d.pos[v] = pos;
}
// ... with the call's parameters among its arguments: the first kernel of a call that is launched directly (nh_call_kernel's prediction)
// brings them along and leaves them in DevParams for the kernels behind it -- no upload in front of the call.
__global__ __launch_bounds__(256) void TETSIM_SFX(nh_predict_value_kernel_)(NHDev d, DevParams pv, DevParams* pdev) {
    if (blockIdx.x == 0u && threadIdx.x == 0u) store_params(pdev, pv);
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= d.nv) return;
    float4 vel = d.vel[v], pos = d.pos[v], prev;
    predict_vertex(load_vparams(pv, v), vel, pos, prev);
    // nh_call_kernel polls prev.w for its own fold's stamp of one substep before, and may look before that store has landed: it then
    // finds this value.  `prev = pos` carries the inverse mass, any non-negative float -- one whose bits equal the awaited stamp was
    // taken for the fold's store (a velocity from the wrong previous position).  0 is no stamp (tetsim_api.hip: next_epoch_block);
    // nothing reads prev.w as a mass.
    prev.w = 0.0f;
    d.vel[v] = vel;
    d.prev[v] = prev;
    d.pos[v] = pos;
}

// Math.max / Math.min (NaN-propagating; -0 < +0).  FAST: the hardware's v_max_f32 / v_min_f32 -- they differ from JavaScript only
// where an operand is NaN or the two are zeros of opposite sign, which the tolerance contract of FAST does not cover (one
// instruction instead of ~10 in the particle passes, which the clustered sweep's first touchers run on their critical chain).
__device__ __forceinline__ T js_max(T a, T b) {
#if TETSIM_FAST
    return __builtin_fmaxf(a, b);
#endif
    if (a != a || b != b) return a + b;  // NaN
    if (a == static_cast<T>(0) && b == static_cast<T>(0)) return __builtin_signbit(a) ? b : a;
    return a > b ? a : b;
}
__device__ __forceinline__ T js_min(T a, T b) {
#if TETSIM_FAST
    return __builtin_fminf(a, b);
#endif
    if (a != a || b != b) return a + b;
    if (a == static_cast<T>(0) && b == static_cast<T>(0)) return __builtin_signbit(a) ? a : b;
    return a < b ? a : b;
}

// bounds / floor friction / grab / velocity, Softbody.js:213-239: (pos, prev) in, (pos, vel) out
// kBodyColliders: the pass also serves body colliders (tetsim_set_body_colliders).  The stepwise kernels do; the one-launch kernels
// (nh_frame_kernel, nh_sweep1_kernel, nh_call_kernel) do not -- with the second list they lose a wave of occupancy or gain a stack -- so
// a body steps through the stepwise kernels while body colliders are on (body.h: nh_frame_now, nh_one_now); they agree bit for bit.
template <bool kBodyColliders = true>
__device__ __forceinline__ void post_vertex(const VParams& P, uint32_t v, float4& pos, const float4& prev, float4& vel) {
    const T dt = P.dt, friction = P.friction;
    const T* lo = P.lo;
    const T* hi = P.hi;
    pos.x = fr(js_max(lo[0], js_min(hi[0], static_cast<T>(pos.x))));  // vecSetClamped :350-355
    pos.y = fr(js_max(lo[1], js_min(hi[1], static_cast<T>(pos.y))));
    pos.z = fr(js_max(lo[2], js_min(hi[2], static_cast<T>(pos.z))));
    if (pos.y < 0.0f) {
        pos.y = 0.0f;
        const float Fx = fr(static_cast<T>(prev.x) - static_cast<T>(pos.x));  // this.F[0], :222
        const float Fz = fr(static_cast<T>(prev.z) - static_cast<T>(pos.z));
        const T m = js_min(static_cast<T>(1.0), dt * friction);
        pos.x = fr(static_cast<T>(pos.x) + static_cast<T>(Fx) * m);
        pos.z = fr(static_cast<T>(pos.z) + static_cast<T>(Fz) * m);
    }
    bool grabbed = static_cast<int32_t>(v) == P.grab_local;
    if (grabbed) { pos.x = P.grab[0]; pos.y = P.grab[1]; pos.z = P.grab[2]; }
    if (P.body_grabs) {   // body grabs (tetsim_set_body_grabs): behind one uniform branch the row of the particle's body decides -- the handle's
                          // grab names nobody then; the row is read through the VALUES of its addresses, before this particle's stores.
                          // Body pins (tetsim_set_body_pins) are the branch's second mode.  Only that mode reads the slots' address, and through
                          // P.all, not as a fourth value of VParams: as a value it cost nh_call_kernel and nh_sweep1_kernel two registers each
                          // (169 and 170 for 167 and 168) and with them a wave per SIMD, for every handle.  So with pins ON the cluster kernels'
                          // write-back loop re-reads that one scalar behind each write-through store, as any_colliders(*P.all) does below
        const int4 row = body_hold_row(P.body_grabs, P.grab_body, P.grab_rows, P.all->pin_slot, v);
        grabbed = row.x == static_cast<int32_t>(v);
        if (grabbed) { pos.x = __int_as_float(row.y); pos.y = __int_as_float(row.z); pos.z = __int_as_float(row.w); }
    }
    if constexpr (kBodyColliders) {
        if (any_colliders(*P.all)) {   // kinematic colliders (collide.h): the handle's list or, with body colliders on, the body's
#if TETSIM_FAST
            collide_particle_f32<true>(pos.x, pos.y, pos.z, prev.x, prev.y, prev.z, *P.all, v, !grabbed);
#else
            collide_particle_f64(pos.x, pos.y, pos.z, prev.x, prev.y, prev.z, *P.all, v, !grabbed);
#endif
        }
    } else if (P.all->n_colliders != 0u && !grabbed) {   // kinematic colliders (collide.h), the handle's list alone
#if TETSIM_FAST
        collide_f32<true>(pos.x, pos.y, pos.z, prev.x, prev.y, prev.z, *P.all);
#else
        collide_f64(pos.x, pos.y, pos.z, prev.x, prev.y, prev.z, *P.all);
#endif
    }
#if TETSIM_FAST
    const T inv_dt = __builtin_amdgcn_rcpf(dt);
#else
    const T inv_dt = static_cast<T>(1.0) / dt;
#endif
    vel.x = fr((static_cast<T>(pos.x) - static_cast<T>(prev.x)) * inv_dt);
    vel.y = fr((static_cast<T>(pos.y) - static_cast<T>(prev.y)) * inv_dt);
    vel.z = fr((static_cast<T>(pos.z) - static_cast<T>(prev.z)) * inv_dt);
    vel.w = 0.0f;
}
__global__ __launch_bounds__(256) void TETSIM_SFX(nh_post_kernel_)(NHDev d) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= d.nv) return;
    float4 pos = d.pos[v], vel;
    post_vertex(load_vparams(*d.params, v), v, pos, d.prev[v], vel);
    d.pos[v] = pos;
    d.vel[v] = vel;
}
// the end of substep s and the prediction of substep s+1 in one pass over the particles (tetsim_step_n, same dt)
__global__ __launch_bounds__(256) void TETSIM_SFX(nh_post_predict_kernel_)(NHDev d) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= d.nv) return;
    float4 pos = d.pos[v], vel, prev;
    const VParams q = load_vparams(*d.params, v);
    post_vertex(q, v, pos, d.prev[v], vel);
    predict_vertex(q, vel, pos, prev);
    store_wt(d.vel, v, vel);
    store_wt(d.prev, v, prev);
    store_wt(d.pos, v, pos);
}

__global__ __launch_bounds__(256) void TETSIM_SFX(nh_post_predict_list_kernel_)(NHDev d, const uint32_t* list, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = list[i];
    float4 pos = d.pos[v], vel, prev;
    const VParams q = load_vparams(*d.params, v);
    post_vertex(q, v, pos, d.prev[v], vel);
    predict_vertex(q, vel, pos, prev);
    store_wt(d.vel, v, vel);
    store_wt(d.prev, v, prev);
    store_wt(d.pos, v, pos);
}
// The particle pass between two substeps of a run, for ONE particle, done by the lane that loads it first in the sweep (kFold
// kernels below): exactly nh_post_predict_kernel's operations on that particle -- the end of the previous substep, then this
// substep's prediction -- so the trajectory is the same bit for bit; velocity and previous position go straight back to memory,
// the predicted position is what the sweep then works on.
template <bool kBodyColliders = true>
__device__ __forceinline__ void fold_particle(const NHDev& d, const VParams& q, uint32_t v, float4& pos, const float4& prev_in) {
    float4 vel, prev;
    post_vertex<kBodyColliders>(q, v, pos, prev_in, vel);
    predict_vertex(q, vel, pos, prev);
    store_wt(d.vel, v, vel);
    store_wt(d.prev, v, prev);
}

// One CLUSTER colour (host_prep.h ClusterPlan): lane = cluster.  The cluster's <= 8 vertices are gathered once into the
// lane's own LDS column, its tets are solved one after the other out of LDS (Gauss-Seidel inside the cluster, in the
// sequential order), and the vertices are written back once: one launch and two memory round trips per cluster colour
// instead of per tet colour.  No barriers: a lane never touches another lane's column, and the clusters of one launch share
// no vertex.  The next tet's streamed data is requested before the current tet is solved.
template <bool kWriteThrough, bool kFold>
__global__ __launch_bounds__(64) void TETSIM_SFX(nh_cluster_kernel_)(NHDev d, NHClusterLaunch L) {
    __shared__ float4 s_pos[kNHClusterVerts * 64];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= L.clusters) return;
    const DevParams& P = *d.params;
    const TetScalars S = tet_scalars(P, L.first[0] + i);
    int32_t vid[kNHClusterVerts];
#pragma unroll
    for (uint32_t k = 0; k < kNHClusterVerts; k++) vid[k] = L.slot_vid[static_cast<size_t>(k) * L.clusters + i];
    uint32_t e = L.first[0] + i;  // step 0 holds every cluster of the launch
    uint32_t cs = d.corner_slots[e];
    float4 ia = d.irp_a[e], ib = d.irp_b[e], ic = d.irp_c[e];
    int32_t ord = d.order[e];
    // UNCONDITIONAL gathers (an unused slot re-reads vertex 0; its LDS cell is never addressed by a corner slot and never
    // written back): inside `if (vid[k] >= 0)` each gather sits in its own branch, the wait-count pass cannot keep a load in
    // flight across the join, and the eight gathers become eight dependent memory round trips (s_waitcnt vmcnt(0) behind
    // every one of them in the round-1 ISA) -- most of what "launch + round trips" cost per cluster colour.
    float4 gathered[kNHClusterVerts];
#pragma unroll
    for (uint32_t k = 0; k < kNHClusterVerts; k++) gathered[k] = d.pos[vid[k] < 0 ? 0 : vid[k]];
    if constexpr (kFold) {
        // first touchers finish the previous substep and predict this one for their particles (previous positions requested with
        // the positions: same round trip)
        const uint32_t mask = L.first_mask[i];
        float4 before[kNHClusterVerts];
#pragma unroll
        for (uint32_t k = 0; k < kNHClusterVerts; k++) before[k] = d.prev[vid[k] < 0 ? 0 : vid[k]];
        const VParams q = load_vparams_of(P, cluster_body(P, L.first[0] + i));   // (only FAST handles fold -- tetsim_create.hip: nh_fold -- the PRECISE fold variants are never launched)
#pragma unroll
        for (uint32_t k = 0; k < kNHClusterVerts; k++)
            if ((mask >> k) & 1u) fold_particle(d, q, static_cast<uint32_t>(vid[k]), gathered[k], before[k]);
    }
#pragma unroll
    for (uint32_t k = 0; k < kNHClusterVerts; k++) s_pos[k * 64u + lane] = gathered[k];
    for (uint32_t j = 0;; j++) {
        const bool more = j + 1u < L.nsteps && i < L.count[j + 1u];
        uint32_t cs_n = 0;
        float4 ia_n = ia, ib_n = ib, ic_n = ic;
        int32_t ord_n = 0;
        if (more) {
            const uint32_t en = L.first[j + 1u] + i;
            cs_n = d.corner_slots[en];
            ia_n = d.irp_a[en]; ib_n = d.irp_b[en]; ic_n = d.irp_c[en];
            ord_n = d.order[en];
        }
        const uint32_t s0 = (cs & 0xffu) * 64u + lane, s1 = ((cs >> 8) & 0xffu) * 64u + lane,
                       s2 = ((cs >> 16) & 0xffu) * 64u + lane, s3 = (cs >> 24) * 64u + lane;
        const float4 q0 = s_pos[s0], q1 = s_pos[s1], q2 = s_pos[s2], q3 = s_pos[s3];
        g3 p[4] = {{q0.x, q0.y, q0.z}, {q1.x, q1.y, q1.z}, {q2.x, q2.y, q2.z}, {q3.x, q3.y, q3.z}};
        const float im[4] = {q0.w, q1.w, q2.w, q3.w};
        const float ir[9] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w, ic.x};
        const T ve = solve_elem(p, im, ir, static_cast<T>(ic.y), S.dt, S.devC, S.volC);
        if (d.vol_err) d.vol_err[ord] = static_cast<double>(ve);
        s_pos[s0] = make_float4(p[0].x, p[0].y, p[0].z, im[0]);  // corner order as in the level kernel
        s_pos[s1] = make_float4(p[1].x, p[1].y, p[1].z, im[1]);
        s_pos[s2] = make_float4(p[2].x, p[2].y, p[2].z, im[2]);
        s_pos[s3] = make_float4(p[3].x, p[3].y, p[3].z, im[3]);
        if (!more) break;
        cs = cs_n; ia = ia_n; ib = ib_n; ic = ic_n; ord = ord_n;
    }
    // write-through: the next launch (other CUs, possibly another XCD) reads these; a plain store would leave the lines dirty
    // in this XCD's L2 until the end-of-kernel write-back (-2.3 us per substep on the 1 M-tet lattice)
#pragma unroll
    for (uint32_t k = 0; k < kNHClusterVerts; k++)
        if (vid[k] >= 0) {
            if constexpr (kWriteThrough) store_wt(d.pos, static_cast<uint32_t>(vid[k]), s_pos[k * 64u + lane]);
            else d.pos[vid[k]] = s_pos[k * 64u + lane];
        }
}

// ---- one cluster on FOUR lanes, one coordinate each -------------------------------------------------------------------------
// A cluster colour is a chain of (tets per cluster) dependent tet solves executed by waves that are alone on their SIMD, and a lone
// wave issues one vector instruction per ~7 cycles (tools/micro/valu_rate.hip; profiles/archive/r02q_nh_persistent_sweep.txt,
// r02s_nh_quad_lanes.txt).  The only lever is fewer instructions per lane.  solveElem's algebra splits by coordinate: with F's
// columns as 3-vectors (matSetMatProduct, Softbody.js:374-379) row c of F, component c of every gradient and of every position
// update depend on component c of the positions alone; the coordinates meet only in three sums per constraint (tr(F^T F), the
// weight w, det F) and in the cross products of the hydrostatic gradient.  So lanes 4q..4q+2 of a quad hold x, y, z of cluster q's
// current tet, lane 4q+3 holds the fourth float of each particle record -- the inverse mass -- and serves it to the others; what
// crosses coordinates goes through quad_perm DPP moves (no LDS, no barrier).
//  FAST: the three sums are re-associated (x + y + z through two DPP adds) and det F is F0 . (F1 x F2): 150 instead of 272 vector
//        instructions per tet and lane; FAST's contract is a tolerance.
//  PRECISE: one lane per cluster on large launches; small ones (<= 2,048 clusters) take the four-lane form below, which gives the same
//        bits -- every lane receives the addends by DPP and adds them up itself in the reference's order -- with the sums, the f64
//        square root and the divisions computed four times over: slower where the launch fills the chip (130.6 against 119.8 us per
//        substep on the 1 M-tet lattice), faster where it is a few waves (the Dragon: 149 -> 103 us).
//  PRECISE on four lanes (the single-workgroup frame kernel of small bodies below, where the chain is everything and lanes are
//        free): every lane receives the addends (f32 values, one DPP move each) and adds them up ITSELF in the reference's order --
//        the sums, the square root and the divisions are computed four times over, the 3x3 products, gradients and position updates
//        once per coordinate -- so the result is solve_elem's, bit for bit.
template <int kCtrl>
__device__ __forceinline__ float quad(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), kCtrl, 0xf, 0xf, true)); }
constexpr int kQuadNext = 0xC9, kQuadNext2 = 0xD2, kQuadLane3 = 0xFF;   // quad_perm [1,2,0,3], [2,0,1,3], [3,3,3,3]
constexpr int kQuadLane0 = 0x00, kQuadLane1 = 0x55, kQuadLane2 = 0xAA;
#if TETSIM_FAST
// (every multiply-add of the FAST four-lane functions is spelled out and nothing else may fuse -- contract(off): the frame kernel
// of small bodies and its stepwise twin inline them in different surroundings and must round alike)
#pragma clang fp contract(off)
__device__ __forceinline__ float sum_xyz(float v) { return v + quad<kQuadNext>(v) + quad<kQuadNext2>(v); }   // lanes 0..2: all three; lane 3: unused
__device__ __forceinline__ float dot3(float a0, float b0, float a1, float b1, float a2, float b2) { return fmaf(a2, b2, fmaf(a1, b1, a0 * b0)); }

// applyToElem (Softbody.js:168-193) for ONE coordinate: g1..g3 in, p updated
__device__ __forceinline__ void apply_coord(float p[4], const float im[4], float g1, float g2, float g3, float C, float alpha) {
    const float g0 = -(g1 + g2 + g3);
    const float w = sum_xyz(fmaf(g3 * g3, im[3], fmaf(g2 * g2, im[2], fmaf(g1 * g1, im[1], g0 * g0 * im[0]))));
    const bool go = C != 0.0f && w != 0.0f;   // the two early returns
    const float dl = -C * __builtin_amdgcn_rcpf(w + alpha);
    p[0] = go ? fmaf(g0, dl * im[0], p[0]) : p[0];
    p[1] = go ? fmaf(g1, dl * im[1], p[1]) : p[1];
    p[2] = go ? fmaf(g2, dl * im[2], p[2]) : p[2];
    p[3] = go ? fmaf(g3, dl * im[3], p[3]) : p[3];
}
__device__ __forceinline__ void f_coord(float F[3], const float p[4], const float ir[9]) {   // row `coordinate` of F = P * invRestPose
    const float P0 = p[1] - p[0], P1 = p[2] - p[0], P2 = p[3] - p[0];
#pragma unroll
    for (int j = 0; j < 3; j++) F[j] = dot3(P0, ir[3 * j], P1, ir[3 * j + 1], P2, ir[3 * j + 2]);
}
// solveElem for one coordinate of one tet; a_dev = devCompliance / dt / dt, a_vol likewise, c_off = volCompliance / devCompliance
__device__ __forceinline__ T solve_quad(float p[4], const float im[4], const float ir[9], T irv, T a_dev, T a_vol, T c_off) {
    float F[3];
    // deviatoric, C = sqrt(tr(F^T F)) (Softbody.js:103-130)
    f_coord(F, p, ir);
    const float r_s2 = sum_xyz(dot3(F[0], F[0], F[1], F[1], F[2], F[2]));
    // (a collapsed tet: r_s2 == 0 -> rsq = inf and 0 * inf = NaN, for which `C != 0` holds and NaNs would be written.  Softbody.js
    // returns early there -- sqrt(0) == 0 == C, :176 -- so C is forced to 0: the NaN gradients are then never selected.)
    const float r_s_inv = __builtin_amdgcn_rsqf(r_s2), r_s = r_s2 > 0.0f ? r_s2 * r_s_inv : 0.0f;
    apply_coord(p, im, dot3(F[0], ir[0], F[1], ir[3], F[2], ir[6]) * r_s_inv, dot3(F[0], ir[1], F[1], ir[4], F[2], ir[7]) * r_s_inv,
                dot3(F[0], ir[2], F[1], ir[5], F[2], ir[8]) * r_s_inv, r_s, a_dev * irv);
    // hydrostatic, C = det F - 1 - volCompliance / devCompliance (:134-165): dF_j = F_{j+1} x F_{j+2}
    f_coord(F, p, ir);
    const float F0n = quad<kQuadNext>(F[0]), F1n = quad<kQuadNext>(F[1]), F2n = quad<kQuadNext>(F[2]);      // component c + 1
    const float F0m = quad<kQuadNext2>(F[0]), F1m = quad<kQuadNext2>(F[1]), F2m = quad<kQuadNext2>(F[2]);   // component c + 2
    const float dF0 = fmaf(F1n, F2m, -(F1m * F2n)), dF1 = fmaf(F2n, F0m, -(F2m * F0n)), dF2 = fmaf(F0n, F1m, -(F0m * F1n));
    const float vol = sum_xyz(F[0] * dF0);
    apply_coord(p, im, dot3(dF0, ir[0], dF1, ir[3], dF2, ir[6]), dot3(dF0, ir[1], dF1, ir[4], dF2, ir[7]), dot3(dF0, ir[2], dF1, ir[5], dF2, ir[8]),
                vol - 1.0f - c_off, a_vol * irv);
    return vol - 1.0f;
}
#pragma clang fp contract(on)
#else
// ---- PRECISE: the scalar code's operations and rounding points (vec_add / vec_diff / cross_store / len2 above), per coordinate
__device__ __forceinline__ void add1(float& a, float b, T scale) { a = fr(static_cast<T>(a) + static_cast<T>(b) * scale); }   // one component of vec_add
__device__ __forceinline__ g3 all_xyz(float v) { g3 r; r.x = quad<kQuadLane0>(v); r.y = quad<kQuadLane1>(v); r.z = quad<kQuadLane2>(v); return r; }
__device__ __forceinline__ void f_coord(float F[3], const float p[4], const float ir[9]) {   // f_from_p for one coordinate
    float Pm[3];
#pragma unroll
    for (int m = 0; m < 3; m++) Pm[m] = fr(static_cast<T>(p[m + 1]) - static_cast<T>(p[0]));   // vec_diff
#pragma unroll
    for (int j = 0; j < 3; j++) {
        F[j] = 0.0f;
        add1(F[j], Pm[0], static_cast<T>(ir[3 * j + 0]));
        add1(F[j], Pm[1], static_cast<T>(ir[3 * j + 1]));
        add1(F[j], Pm[2], static_cast<T>(ir[3 * j + 2]));
    }
}
// apply_to_elem for one coordinate: g[1..3] in.  C, w and dlambda come out identical in the four lanes of a quad (they are
// functions of broadcast values only), so the two early returns are quad-uniform and the DPP moves never meet a masked lane.
__device__ __forceinline__ void apply_coord(float p[4], const float im[4], float g[4], T C, T alpha) {
    if (C == static_cast<T>(0)) return;
    g[0] = 0.0f;
    add1(g[0], g[1], static_cast<T>(-1.0));
    add1(g[0], g[2], static_cast<T>(-1.0));
    add1(g[0], g[3], static_cast<T>(-1.0));
    T w = static_cast<T>(0);
#pragma unroll
    for (int i = 0; i < 4; i++) w += len2(all_xyz(g[i])) * static_cast<T>(im[i]);
    if (w == static_cast<T>(0)) return;
    const T dlambda = -C / (w + alpha);
#pragma unroll
    for (int i = 0; i < 4; i++) add1(p[i], g[i], dlambda * static_cast<T>(im[i]));
}
__device__ __forceinline__ T solve_quad(float p[4], const float im[4], const float ir[9], T irv, T a_dev, T a_vol, T c_off) {
    float F[3], g[4];
    // deviatoric (solve_elem above, line for line)
    f_coord(F, p, ir);
    const T r_s = sqrt_(len2(all_xyz(F[0])) + len2(all_xyz(F[1])) + len2(all_xyz(F[2])));
    const T r_s_inv = static_cast<T>(1.0) / r_s;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        g[k + 1] = 0.0f;
        add1(g[k + 1], F[0], r_s_inv * static_cast<T>(ir[3 * 0 + k]));
        add1(g[k + 1], F[1], r_s_inv * static_cast<T>(ir[3 * 1 + k]));
        add1(g[k + 1], F[2], r_s_inv * static_cast<T>(ir[3 * 2 + k]));
    }
    apply_coord(p, im, g, r_s, a_dev * irv);
    // hydrostatic
    f_coord(F, p, ir);
    const g3 f0 = all_xyz(F[0]), f1 = all_xyz(F[1]), f2 = all_xyz(F[2]);
    // cross_store for component c: r.c = b[c+1] * c[c+2] - b[c+2] * c[c+1] (cyclic, :343-348)
    auto cross1 = [](float b_next, float c_next2, float b_next2, float c_next) {
        return fr(static_cast<T>(b_next) * static_cast<T>(c_next2) - static_cast<T>(b_next2) * static_cast<T>(c_next));
    };
    const float F0n = quad<kQuadNext>(F[0]), F1n = quad<kQuadNext>(F[1]), F2n = quad<kQuadNext>(F[2]);
    const float F0m = quad<kQuadNext2>(F[0]), F1m = quad<kQuadNext2>(F[1]), F2m = quad<kQuadNext2>(F[2]);
    const float dF0 = cross1(F1n, F2m, F1m, F2n), dF1 = cross1(F2n, F0m, F2m, F0n), dF2 = cross1(F0n, F1m, F0m, F1n);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        g[k + 1] = 0.0f;
        add1(g[k + 1], dF0, static_cast<T>(ir[3 * 0 + k]));
        add1(g[k + 1], dF1, static_cast<T>(ir[3 * 1 + k]));
        add1(g[k + 1], dF2, static_cast<T>(ir[3 * 2 + k]));
    }
    T vol;
    {  // matGetDeterminant(F) :381-387, term order as written
        const T a11 = f0.x, a12 = f1.x, a13 = f2.x;
        const T a21 = f0.y, a22 = f1.y, a23 = f2.y;
        const T a31 = f0.z, a32 = f1.z, a33 = f2.z;
        vol = a11 * a22 * a33 + a12 * a23 * a31 + a13 * a21 * a32 - a13 * a22 * a31 - a12 * a21 * a33 - a11 * a23 * a32;
    }
    apply_coord(p, im, g, vol - static_cast<T>(1.0) - c_off, a_vol * irv);
    return vol - static_cast<T>(1.0);
}
#endif  // TETSIM_FAST / PRECISE quad functions

// ---- SMALL bodies: a whole call as ONE workgroup, every particle in LDS, one tet on four lanes --------------------------------
// The reference's own workload (the Dragon: 1,234 particles, 3,840 tets; main.js:26-27, Softbody.js:195-240) is 34 launches per
// substep with the level kernels above -- 32 colours of ~120 tets, each a launch boundary (~1.9 us) plus two dependent memory round
// trips around ~1 us of arithmetic.  Here one workgroup keeps positions + inverse masses (16 B), previous positions and velocities
// (12 B each) of ALL particles in LDS (160 KB per CU: 4,096 particles), walks the levels of the solve order with a workgroup barrier
// between them and the substeps of the call one after the other; a tet's streamed record (ids, inverse rest pose, 1 / rest volume)
// for the NEXT level is requested before the current one is solved.  What is left of a level is the dependent chain of ONE tet
// solve, so the tets of a NARROW level (<= kNHQuadLevel) are solved by a quad of lanes each, one coordinate per lane (solve_quad);
// wide levels keep one lane per tet (solve_elem): four times the waves on one CU's SIMDs would cost what the shorter chain saves.
// PRECISE: both forms give the same bits, the reference's.  FAST: solve_quad re-associates at tolerance level; the stepwise twin
// (tetsim_profile) makes the same choice per level -- nh_level4_kernel is solve_quad from memory -- so the two agree bit for bit.
#if TETSIM_FAST
constexpr uint32_t kNHQuadLevel = kNHQuadLevelFast;
#else
constexpr uint32_t kNHQuadLevel = kNHQuadLevelPrecise;
#endif
struct NHTetRecord { int4 id; float4 a, b, c; };
__device__ __forceinline__ NHTetRecord nh_load_record(const NHDev& d, uint32_t e) {
    NHTetRecord r;
    r.id = d.tet_idx[e]; r.a = d.irp_a[e]; r.b = d.irp_b[e]; r.c = d.irp_c[e];
    return r;
}
// one tet on the quad's four lanes out of a float4 particle array `sp` (LDS or memory): lane c works on float c of every record
__device__ __forceinline__ T nh_solve_record_quad(float* const sp, const NHTetRecord& r, uint32_t c, const QuadScalars& Q) {
    const uint32_t a0 = 4u * static_cast<uint32_t>(r.id.x) + c, a1 = 4u * static_cast<uint32_t>(r.id.y) + c,
                   a2 = 4u * static_cast<uint32_t>(r.id.z) + c, a3 = 4u * static_cast<uint32_t>(r.id.w) + c;
    float p[4] = {sp[a0], sp[a1], sp[a2], sp[a3]};   // lanes 0..2: a coordinate; lane 3: the inverse masses
    const float im[4] = {quad<kQuadLane3>(p[0]), quad<kQuadLane3>(p[1]), quad<kQuadLane3>(p[2]), quad<kQuadLane3>(p[3])};
    const float ir[9] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.c.x};
    const T ve = solve_quad(p, im, ir, static_cast<T>(r.c.y), Q.a_dev, Q.a_vol, Q.c_off);
    if (c < 3u) { sp[a0] = p[0]; sp[a1] = p[1]; sp[a2] = p[2]; sp[a3] = p[3]; }   // (lane 3 leaves the inverse masses alone)
    return ve;
}
// One workgroup per BODY of the handle (tetsim_create_batch: independent bodies; a plain body is a batch of one).  seg: per level and
// body the (first, end) solve positions of the body's tets, [levels][bodies][2] (the tets of a level are laid out body by body);
// first_vert: [bodies + 1].  The call's parameters arrive by value, with the launch (no upload in front of a call; the first workgroup
// leaves them in DevParams for the kernels behind this one).
__global__ __launch_bounds__(512) void TETSIM_SFX(nh_frame_kernel_)(NHDev d, const uint32_t* __restrict__ seg, const uint32_t* __restrict__ first_vert,
                                                                   uint32_t levels, uint32_t bodies, uint32_t n, DevParams pv, DevParams* pdev) {
    if (blockIdx.x == 0u && threadIdx.x == 0u) store_params(pdev, pv);
    extern __shared__ float4 s_frame[];
    const uint32_t body = blockIdx.x, vbase = first_vert[body], nvb = first_vert[body + 1u] - vbase;
    float4* const s_pos = s_frame;                                        // [nvb] xyz + inverse mass
    float* const s_prev = reinterpret_cast<float*>(s_frame + nvb);        // [3 nvb]
    float* const s_vel = s_prev + 3ull * nvb;                             // [3 nvb]
    float* const sp = reinterpret_cast<float*>(s_frame);
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, c = tid & 3u, qd = tid >> 2, nq = nthr >> 2;
    const DevParams& P = pv;
    TetScalars S = tet_scalars(P);
    body_compliances_of(P, body, S.devC, S.volC);   // (one workgroup per body: the row arrives through scalar loads)
    const QuadScalars Q = quad_scalars(S);
    const VParams q = load_vparams_of(P, body);
    for (uint32_t v = tid; v < nvb; v += nthr) {   // the call starts with a prediction (Softbody.js:198-202), as enqueue_substep(first) does
        float4 pos = d.pos[vbase + v], vel = d.vel[vbase + v], prev;
        predict_vertex(q, vel, pos, prev);
        s_pos[v] = pos;
        s_prev[3u * v] = prev.x; s_prev[3u * v + 1u] = prev.y; s_prev[3u * v + 2u] = prev.z;
        s_vel[3u * v] = vel.x; s_vel[3u * v + 1u] = vel.y; s_vel[3u * v + 2u] = vel.z;
    }
    // (a level's bounds are scalar loads on its critical chain: the next level's are requested while this one is solved)
    const uint2* const my_seg = reinterpret_cast<const uint2*>(seg) + body;   // (first, end) of this body's piece of level l at [l * bodies]
    const uint32_t pitch = bodies;
    const uint2 seg_first = levels != 0u ? my_seg[0] : make_uint2(0u, 0u);
    const uint32_t lo_first = seg_first.x, hi_first = seg_first.y;
    // A level of at most kNHQuadLevel tets is solved on four lanes per tet (its chain is all there is: fewer instructions per lane);
    // a wider one keeps one lane per tet (four times the waves on ONE CU's SIMDs would cost what the shorter chain saves).
    auto on_quads = [](uint32_t count) { return count <= kNHQuadLevel; };
    auto load_local = [&](uint32_t e) { return nh_load_record(d, e); };   // (corner ids stay global until they are used: nothing may wait for a record requested ahead)
    NHTetRecord rec;
    uint32_t rec_e = 0xffffffffu;   // the solve position `rec` holds (the four lanes of a quad hold the same record on a four-lane level)
    if (levels != 0u) {
        const uint32_t e = lo_first + (on_quads(hi_first - lo_first) ? qd : tid);
        if (e < hi_first) { rec_e = e; rec = load_local(e); }
    }
    __syncthreads();
    uint32_t lo_next = lo_first, hi_next = hi_first;
    for (uint32_t s = 0; s < n; s++) {
        for (uint32_t l = 0; l < levels; l++) {
            const uint32_t lo = lo_next, hi = hi_next;
            if (l + 1u < levels) { const uint2 nx = my_seg[static_cast<size_t>(l + 1u) * pitch]; lo_next = nx.x; hi_next = nx.y; }   // (one 8-byte scalar load)
            else { lo_next = lo_first; hi_next = hi_first; }   // (behind the last level: the next substep's first)
            const bool quads = on_quads(hi - lo);
            const uint32_t me = quads ? qd : tid, stride = quads ? nq : nthr;
            const uint32_t me_n = on_quads(hi_next - lo_next) ? qd : tid;
            for (uint32_t e0 = lo; e0 < hi; e0 += stride) {   // (uniform)
                const uint32_t e = e0 + me;
                const bool valid = e < hi;   // (whole quads on a four-lane level)
                if (valid && rec_e != e) { rec = load_local(e); rec_e = e; }   // (not requested ahead: only behind an empty level)
                NHTetRecord cur = rec;
                {   // this lane's next tet: further down this level, else its position in the next level
                    uint32_t ne = e + stride;
                    bool more = e0 + stride < hi && ne < hi;
                    if (e0 + stride >= hi) {
                        ne = lo_next + me_n;
                        more = (l + 1u < levels || s + 1u < n) && ne < hi_next;
                    }
                    if (more) { rec = load_local(ne); rec_e = ne; }
                }
                if (valid) {
                    // the corners as indices into this body's LDS arrays
                    cur.id.x -= static_cast<int32_t>(vbase); cur.id.y -= static_cast<int32_t>(vbase); cur.id.z -= static_cast<int32_t>(vbase); cur.id.w -= static_cast<int32_t>(vbase);
                    T ve;
                    if (quads) ve = nh_solve_record_quad(sp, cur, c, Q);
                    else {
                        const float4 q0 = s_pos[cur.id.x], q1 = s_pos[cur.id.y], q2 = s_pos[cur.id.z], q3 = s_pos[cur.id.w];
                        g3 p[4] = {{q0.x, q0.y, q0.z}, {q1.x, q1.y, q1.z}, {q2.x, q2.y, q2.z}, {q3.x, q3.y, q3.z}};
                        const float im[4] = {q0.w, q1.w, q2.w, q3.w};
                        const float ir[9] = {cur.a.x, cur.a.y, cur.a.z, cur.a.w, cur.b.x, cur.b.y, cur.b.z, cur.b.w, cur.c.x};
                        ve = solve_elem(p, im, ir, static_cast<T>(cur.c.y), S.dt, S.devC, S.volC);
                        s_pos[cur.id.x] = make_float4(p[0].x, p[0].y, p[0].z, im[0]);
                        s_pos[cur.id.y] = make_float4(p[1].x, p[1].y, p[1].z, im[1]);
                        s_pos[cur.id.z] = make_float4(p[2].x, p[2].y, p[2].z, im[2]);
                        s_pos[cur.id.w] = make_float4(p[3].x, p[3].y, p[3].z, im[3]);
                    }
                    if (s + 1u == n && (!quads || c == 0u)) d.vol_err[d.order[e]] = static_cast<double>(ve);   // (what the call leaves behind: its last sweep's)
                }
            }
            __syncthreads();
        }
        // bounds, floor, grab, velocity (Softbody.js:213-239) and, between two substeps, the next prediction: one pass over the particles
        const bool last = s + 1u == n;
        for (uint32_t v = tid; v < nvb; v += nthr) {
            float4 pos = s_pos[v], vel;
            float4 prev = make_float4(s_prev[3u * v], s_prev[3u * v + 1u], s_prev[3u * v + 2u], 0.0f);
            post_vertex<false>(q, vbase + v, pos, prev, vel);
            if (!last) {
                predict_vertex(q, vel, pos, prev);
                s_pos[v] = pos;
                s_prev[3u * v] = prev.x; s_prev[3u * v + 1u] = prev.y; s_prev[3u * v + 2u] = prev.z;
                s_vel[3u * v] = vel.x; s_vel[3u * v + 1u] = vel.y; s_vel[3u * v + 2u] = vel.z;
            } else {
                d.pos[vbase + v] = pos;
                d.vel[vbase + v] = vel;
                d.prev[vbase + v] = make_float4(prev.x, prev.y, prev.z, pos.w);   // (the level kernels' `prev = pos` carries the inverse mass along)
            }
        }
        __syncthreads();
    }
}
// One level, one tet per quad, particles in memory: the stepwise twin of the frame kernel's FAST sweep (tetsim_profile on such a body),
// and the level kernel of bodies whose levels are a few waves (nh_sweep)
__global__ __launch_bounds__(256) void TETSIM_SFX(nh_level4_kernel_)(NHDev d, uint32_t first, uint32_t count) {
    const uint32_t i = (blockIdx.x * 256u + threadIdx.x) >> 2, c = threadIdx.x & 3u;
    if (i >= count) return;   // (whole quads)
    const uint32_t e = first + i;
    const QuadScalars Q = quad_scalars(tet_scalars(*d.params, e));
    const T ve = nh_solve_record_quad(reinterpret_cast<float*>(d.pos), nh_load_record(d, e), c, Q);
    if (c == 0u && d.vol_err) d.vol_err[d.order[e]] = static_cast<double>(ve);
}

// ---- the steps of one cluster on four lanes ------------------------------------------------------------------------------------------
// Three kernels execute a cluster this way and promise each other's bits: nh_cluster4_kernel (one launch per colour), nh_sweep1_kernel
// (per substep) and nh_call_kernel (per call).  nh_cluster4_kernel and nh_sweep1_kernel take the steps they share from ONE routine
// each: which cluster and coordinate a lane is (quad_lane), the solve's scalars (tet_scalars, quad_scalars above), the tets' streamed
// records (ClusterRecords, cluster_tet), the chain of solves out of LDS (solve_cluster_steps) and the particle pass of a first toucher
// (fold_particle above); the sweep also the colour of a block (find_colour) and a look at a handed-on particle (take_stamped).
// nh_call_kernel is NOT built from them: it keeps every one of these steps WRITTEN OUT, kept equal to the routines by hand.  Built from
// them it has the same registers, LDS and waves and is 124 bytes shorter, and a substep of the 1 M-tet lattice costs 0.1-0.4 % more in
// four sessions of five; no single routine accounts for it, only the kernel with every step written out measures as before
// (profiles/nh_cluster_refactor.txt, sections 5 to 7).  A change to a routine below is therefore made a second time in nh_call_kernel;
// tests/test_gpu_nh_cluster_paths_golden.py and the twin tests hold the two to each other's bits.  Also kept in each kernel: the ORDER in
// which its loads are issued with the barriers that hold it, the polling loop and the stamped hand-over tail of the two one-launch kernels.
// Lane `lane` of a wave works on coordinate c (3: the inverse masses) of the wave's cluster cl, which is cluster i of its colour; `block`
// counts from the colour's first block.  s_pos: the wave's own LDS slice [vertex slot][cluster of the wave] -- four independent waves per
// workgroup, no barrier anywhere.  (A lane with i >= clusters leaves at once, in whole quads: the DPP moves stay inside a quad.)
struct QuadLane { float4* s_pos; uint32_t lane, c, cl, i; };
__device__ __forceinline__ QuadLane quad_lane(float4 (*s_all)[kNHClusterVerts * 16], uint32_t block) {
    const uint32_t lane = threadIdx.x & 63u;
    return {s_all[threadIdx.x >> 6], lane, lane & 3u, lane >> 2, (block * 4u + (threadIdx.x >> 6)) * 16u + (lane >> 2)};
}
// The tet of step j of cluster i: a step the cluster does not have names its first tet.  The two routines say the same; which one a
// kernel takes decides what the compiler makes of it, and the kernels keep what they had before these routines existed.  Where L is a
// kernel argument (nh_cluster4_kernel) first[] sits in scalar registers: both sums are formed and one is chosen.  Where L lies in memory
// (the one-launch kernels' colour table) the choice is made between the two READS of first[]: one load at a lane-dependent address,
// which this step's records then wait for.  (Written as the one expression below, the kernel-argument case came out either way,
// depending on the code around it.)  The forms are NOT interchangeable in speed: with the select form nh_call_kernel measures 0.858
// against 0.833 ms per 20 substeps on the 1 M-tet lattice, five pairs (profiles/nh_cluster_refactor.txt, which also shows how to tell
// the forms apart in the assembly: a global_load_dword and s_waitcnt vmcnt(0) in front of every step's five record loads, or none).
__device__ __forceinline__ uint32_t cluster_tet(const NHClusterLaunch& L, uint32_t i, uint32_t j) {
    return (j < L.nsteps && i < L.count[j]) ? L.first[j] + i : L.first[0] + i;
}
__device__ __forceinline__ uint32_t cluster_tet_of_arguments(const NHClusterLaunch& L, uint32_t i, uint32_t j) {
    const uint32_t e_j = L.first[j] + i, e_0 = L.first[0] + i;
    return (j < L.nsteps && i < L.count[j]) ? e_j : e_0;
}
// The streamed records of the cluster's tets.  Order of issue in every kernel (vmcnt retires in order): ids and the FIRST tet's record,
// then -- as soon as the ids are here -- the particles, then every other tet's record, unconditionally (a step this cluster does not
// have re-reads its first tet).  The first solve starts when the particles land while the later records stream in.  The kernels hold
// that order with a sched_barrier behind request(0), behind the particles and behind request(1..7): left alone, the scheduler issues
// ids -> particles -> records, three dependent trips.
struct ClusterRecords {
    uint32_t cs[kNHClusterTets];
    float4 ia[kNHClusterTets], ib[kNHClusterTets], ic[kNHClusterTets];
    int32_t ord[kNHClusterTets];
    __device__ __forceinline__ void request(const NHDev& d, uint32_t j, uint32_t e) {   // e: cluster_tet
        cs[j] = d.corner_slots[e];
        ia[j] = d.irp_a[e]; ib[j] = d.irp_b[e]; ic[j] = d.irp_c[e];
        ord[j] = d.order[e];
    }
};
// The cluster's tets one after the other out of the wave's LDS slice (Gauss-Seidel inside the cluster, in the sequential order): one wave
// per slice and the LDS operations of a wave execute in order, so no barrier.  store_vol_err: this sweep's volError is what the call
// leaves behind (the call kernel: its last substep's only).
__device__ __forceinline__ void solve_cluster_steps(const QuadLane& q, const NHClusterLaunch& L, const ClusterRecords& r, const QuadScalars& Q,
                                                    const NHDev& d, bool store_vol_err) {
    float* const sp = reinterpret_cast<float*>(q.s_pos) + q.lane;   // this lane's float of slot 0; slot s is 64 floats on per s
#pragma unroll
    for (uint32_t j = 0; j < kNHClusterTets; j++) {
        if (j >= L.nsteps) break;            // (uniform)
        if (q.i < L.count[j]) {              // (counts do not increase with j; whole quads agree)
            // float index of (slot, cl, c) = slot * 64 + lane: one field extraction and one add per corner
            const uint32_t a0 = (r.cs[j] << 6) & 0x3fc0u, a1 = (r.cs[j] >> 2) & 0x3fc0u, a2 = (r.cs[j] >> 10) & 0x3fc0u, a3 = (r.cs[j] >> 18) & 0x3fc0u;
            float p[4] = {sp[a0], sp[a1], sp[a2], sp[a3]};   // lanes 0..2: a coordinate; lane 3: the inverse masses
            const float im[4] = {quad<kQuadLane3>(p[0]), quad<kQuadLane3>(p[1]), quad<kQuadLane3>(p[2]), quad<kQuadLane3>(p[3])};
            const float ir[9] = {r.ia[j].x, r.ia[j].y, r.ia[j].z, r.ia[j].w, r.ib[j].x, r.ib[j].y, r.ib[j].z, r.ib[j].w, r.ic[j].x};
            const T ve = solve_quad(p, im, ir, static_cast<T>(r.ic[j].y), Q.a_dev, Q.a_vol, Q.c_off);
            if (q.c == 0u && d.vol_err && store_vol_err) d.vol_err[r.ord[j]] = static_cast<double>(ve);
            if (q.c < 3u) { sp[a0] = p[0]; sp[a1] = p[1]; sp[a2] = p[2]; sp[a3] = p[3]; }   // (lane 3 leaves the inverse masses alone)
        }
    }
}

// The first five arguments repeat what the first memory trips need (ids, particles, mask, count) as plain scalars in front of the
// structs: scalars can be PRELOADED into SGPRs when the wave starts (the unit is built with -amdgpu-kernarg-preload-count), structs
// passed by value cannot -- the kernel-argument load is then off the chain "arguments -> ids -> particles" of every colour.
template <bool kWriteThrough, bool kFold>
__global__ __launch_bounds__(256) void TETSIM_SFX(nh_cluster4_kernel_)(const int32_t* __restrict__ a_slot_vid, const float4* __restrict__ a_pos,
                                                               const uint8_t* __restrict__ a_first_mask, const float4* __restrict__ a_prev,
                                                               uint32_t a_clusters, NHDev d, NHClusterLaunch L) {
    __shared__ float4 s_all[4][kNHClusterVerts * 16];
    const QuadLane q = quad_lane(s_all, blockIdx.x);
    float4* const s_pos = q.s_pos;
    const uint32_t c = q.c, cl = q.cl, i = q.i;
    if (i >= a_clusters) return;
    const DevParams& P = *d.params;
    const QuadScalars Q = quad_scalars(tet_scalars(P, L.first[0] + i));
    // the cluster's <= 8 particles: lane c fetches slots c and c + 4 (unconditionally, see nh_cluster_kernel) and writes them back
    const int32_t va = a_slot_vid[static_cast<size_t>(c) * a_clusters + i], vb = a_slot_vid[static_cast<size_t>(c + 4u) * a_clusters + i];
    [[maybe_unused]] uint32_t fmask = 0;
    if constexpr (kFold) fmask = a_first_mask[i];
    ClusterRecords rec;
    rec.request(d, 0, cluster_tet_of_arguments(L, i, 0));
    __builtin_amdgcn_sched_barrier(0);
    float4 ga = a_pos[va < 0 ? 0 : va], gb = a_pos[vb < 0 ? 0 : vb];
    [[maybe_unused]] float4 pa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pb = pa;
    if constexpr (kFold) {
        // (only the lanes with a first touch ask for previous positions -- behind the positions, in the same round trip; on the
        // lattice that is every lane of the first colour and a few waves along the faces in the others)
        if ((fmask >> c) & 1u) pa = a_prev[va];
        if ((fmask >> (c + 4u)) & 1u) pb = a_prev[vb];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (uint32_t j = 1; j < kNHClusterTets; j++) rec.request(d, j, cluster_tet_of_arguments(L, i, j));
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (kFold) {
        // the lane that loads a particle the cluster touches first finishes the previous substep and predicts this one for it (whole
        // particles, two per lane: the per-coordinate split starts behind this)
        if (fmask & (0x11u << c)) {
            const VParams vp = load_vparams_of(P, cluster_body(P, L.first[0] + i));
            if ((fmask >> c) & 1u) fold_particle(d, vp, static_cast<uint32_t>(va), ga, pa);
            if ((fmask >> (c + 4u)) & 1u) fold_particle(d, vp, static_cast<uint32_t>(vb), gb, pb);
        }
    }
    s_pos[c * 16u + cl] = ga;
    s_pos[(c + 4u) * 16u + cl] = gb;
    solve_cluster_steps(q, L, rec, Q, d, true);
    if (va >= 0) { if constexpr (kWriteThrough) store_wt(d.pos, static_cast<uint32_t>(va), s_pos[c * 16u + cl]); else d.pos[va] = s_pos[c * 16u + cl]; }
    if (vb >= 0) { if constexpr (kWriteThrough) store_wt(d.pos, static_cast<uint32_t>(vb), s_pos[(c + 4u) * 16u + cl]); else d.pos[vb] = s_pos[(c + 4u) * 16u + cl]; }
}

#if TETSIM_FAST
// ---- the clustered sweep as ONE launch: all colours in one grid, particles handed on with their stamp (dev_common.h: NHSweep) -------
// nh_cluster4_kernel's cluster on four lanes, operation for operation -- the solves are solve_cluster_steps there and here, on the same
// inputs, and the particle pass of a first toucher is fold_particle, so the sweep equals the one-launch-per-colour sweep bit for bit --
// with three differences around it:
//   * a wave finds its colour from its block index (scalar search over <= 255 colours) and reads that colour's descriptor;
//   * a slot whose particle an EARLIER colour of this sweep touched is polled from the exchange array until it carries the stamp of that
//     colour (memory-side loads: the writer may sit on another XCD, and no kernel boundary lies between the two); first touches come
//     from NHDev::pos as before (with the folded particle pass between two substeps);
//   * a slot's result goes to the exchange array with this colour's stamp -- or, when no later cluster touches the particle, to
//     NHDev::pos with its inverse mass, where the particle kernels, the next substep's first touchers and the read-backs expect it.
// Eight launch boundaries and ramps per substep become one.  Waits are bounded (timeout_ms; *error says so at the next tetsim_sync).
// The colour of block `block` of a sweep: a uniform search over the colours' first blocks.
__device__ __forceinline__ uint32_t find_colour(const NHSweepColour* __restrict__ cols, uint32_t ncol, uint32_t block) {
    uint32_t k = 0;
    while (k + 1u < ncol && block >= cols[k + 1u].first_block) k++;   // (uniform)
    return k;
}
// A look at a handed-on particle: it is taken once it carries the stamp of the colour that wrote it.
__device__ __forceinline__ void take_stamped(const float4& x, uint32_t want, float4& g, bool& pend) {
    if (pend && __float_as_uint(x.w) == want) { g = x; pend = false; }
}
template <bool kFold>
__global__ __launch_bounds__(256) void nh_sweep1_kernel(const NHSweepColour* __restrict__ cols, uint32_t ncol, float4* xch, uint32_t sub_index, uint32_t epoch_arg,
                                                        uint32_t* err, uint32_t timeout_ms, NHDev d) {
    __shared__ float4 s_all[4][kNHClusterVerts * 16];
    const uint32_t k = find_colour(cols, ncol, blockIdx.x);
    const NHSweepColour& C = cols[k];
    const NHClusterLaunch& L = C.L;
    const QuadLane q = quad_lane(s_all, blockIdx.x - C.first_block);
    float4* const s_pos = q.s_pos;
    const uint32_t c = q.c, cl = q.cl, i = q.i;
    const uint32_t clusters = L.clusters;
    if (i >= clusters) return;
    const DevParams& P = *d.params;
    const QuadScalars Q = quad_scalars(tet_scalars(P, L.first[0] + i));
    const uint32_t stamp = (epoch_arg ? epoch_arg : P.epoch) + sub_index * ncol + k + 1u;
    const int32_t va = L.slot_vid[static_cast<size_t>(c) * clusters + i], vb = L.slot_vid[static_cast<size_t>(c + 4u) * clusters + i];
    const float ima = C.slot_im[static_cast<size_t>(c) * clusters + i], imb = C.slot_im[static_cast<size_t>(c + 4u) * clusters + i];
    const uint2 dl = C.delta[i];
    const uint32_t lmask = C.last_mask[i];
    [[maybe_unused]] uint32_t fmask = 0;
    if constexpr (kFold) fmask = L.first_mask[i];
    ClusterRecords rec;
    rec.request(d, 0, cluster_tet(L, i, 0));
    __builtin_amdgcn_sched_barrier(0);
    // slot c -> byte c of dl.x, slot c + 4 -> byte c of dl.y: 0 = first touch of the sweep
    const uint32_t da = (dl.x >> (8u * c)) & 0xffu, db = (dl.y >> (8u * c)) & 0xffu;
    const uint32_t want_a = stamp - da, want_b = stamp - db;
    const uint32_t ua = va < 0 ? 0u : static_cast<uint32_t>(va), ub = vb < 0 ? 0u : static_cast<uint32_t>(vb);
    bool pend_a = va >= 0 && da != 0u, pend_b = vb >= 0 && db != 0u;
    // first look: everything in one trip (a first touch reads NHDev::pos, a handed-on particle the exchange array past the caches)
    float4 ga = d.pos[ua], gb = d.pos[ub];
    float4 xa = load_coherent(xch, ua), xb = load_coherent(xch, ub);
    [[maybe_unused]] float4 pa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pb = pa;
    if constexpr (kFold) {
        if ((fmask >> c) & 1u) pa = d.prev[ua];
        if ((fmask >> (c + 4u)) & 1u) pb = d.prev[ub];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (uint32_t j = 1; j < kNHClusterTets; j++) rec.request(d, j, cluster_tet(L, i, j));
    __builtin_amdgcn_sched_barrier(0);
    take_stamped(xa, want_a, ga, pend_a);
    take_stamped(xb, want_b, gb, pend_b);
    if (__builtin_amdgcn_ballot_w64(pend_a || pend_b) != 0ull) {
        const long long t0 = wall_clock64(), limit = 100000ll * timeout_ms;   // 100 MHz ticks; 0 = unbounded
        do {
            __builtin_amdgcn_s_sleep(TETSIM_NH_POLL_SLEEP);
            // (other workgroups write the exchange array while this one looks: every look is a fresh load -- declared __restrict__, with no
            // store to it inside the loop, the first build's looks were folded into the one in front of the loop and waited for ever)
            asm volatile("" ::: "memory");
            if (pend_a) take_stamped(load_coherent(xch, ua), want_a, ga, pend_a);
            if (pend_b) take_stamped(load_coherent(xch, ub), want_b, gb, pend_b);
            if (limit && (pend_a || pend_b) && wall_clock64() - t0 > limit) {   // never in a correct run; a wedged GPU helps nobody
                __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                pend_a = pend_b = false;
            }
        } while (__builtin_amdgcn_ballot_w64(pend_a || pend_b) != 0ull);
    }
    if constexpr (kFold) {
        if (fmask & (0x11u << c)) {
            const VParams vp = load_vparams_of(P, cluster_body(P, L.first[0] + i));
            if ((fmask >> c) & 1u) fold_particle<false>(d, vp, ua, ga, pa);
            if ((fmask >> (c + 4u)) & 1u) fold_particle<false>(d, vp, ub, gb, pb);
        }
    }
    ga.w = ima; gb.w = imb;   // the inverse masses (lane 3 of a quad reads them from the fourth float below)
    s_pos[c * 16u + cl] = ga;
    s_pos[(c + 4u) * 16u + cl] = gb;
    solve_cluster_steps(q, L, rec, Q, d, true);
    // A slot's result leaves the cluster: to NHDev::pos with its inverse mass where no later cluster of the sweep touches the particle, else
    // to the exchange array with this colour's stamp in the fourth float.  (Not a function: behind one the compiler merges the two stores
    // into one at a lane-dependent base, a loop over the bases present in the wave, and this kernel loses a wave.)
    if (va >= 0) {
        float4 r = s_pos[c * 16u + cl];
        if ((lmask >> c) & 1u) store_wt(d.pos, ua, r);
        else { r.w = __uint_as_float(stamp); store_wt(xch, ua, r); }
    }
    if (vb >= 0) {
        float4 r = s_pos[(c + 4u) * 16u + cl];
        if ((lmask >> (c + 4u)) & 1u) store_wt(d.pos, ub, r);
        else { r.w = __uint_as_float(stamp); store_wt(xch, ub, r); }
    }
}

// ---- a whole CALL as one launch: the sweeps of all n substeps in one grid (clustered FAST bodies whose every particle some cluster touches) --
// nh_sweep1_kernel with the hand-over carried across substeps: the sweep's LAST toucher of a particle hands it to the next substep's FIRST
// toucher through the exchange array too (stamp of its own colour in its own substep; the host's delta_first says how far back that is),
// the first toucher does the particle pass between the two substeps as it takes the particle over (fold_particle's operations; the previous
// position it needs was stored by itself one substep earlier, stamped, and is read past the caches), and only the call's last substep
// stores to NHDev::pos and volError.  One launch boundary per CALL instead of per substep; colour 0 of a substep starts wherever the
// clusters around it have finished the substep before.  Same arithmetic in the same order: bit-equal to the per-substep launches.  (Every
// step is written out here, not taken from the shared routines above: see the note in front of quad_lane.)
__global__ __launch_bounds__(256) void nh_call_kernel(const NHSweepColour* __restrict__ cols, uint32_t ncol, float4* xch, uint32_t n_sub, uint32_t blocks_per_sub, uint32_t blocks,
                                                      uint32_t* err, uint32_t timeout_ms, NHDev d) {
    __shared__ float4 s_all[4][kNHClusterVerts * 16];
    const uint32_t sub = blockIdx.x / blocks_per_sub, r = blockIdx.x - sub * blocks_per_sub;
    if (r >= blocks) return;   // (padding: a substep's blocks are a multiple of 8)
    uint32_t k = 0;
    while (k + 1u < ncol && r >= cols[k + 1u].first_block) k++;   // (uniform)
    const NHSweepColour& C = cols[k];
    const NHClusterLaunch& L = C.L;
    float4* const s_pos = s_all[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u, c = lane & 3u, cl = lane >> 2, i = ((r - C.first_block) * 4u + (threadIdx.x >> 6)) * 16u + cl;
    const uint32_t clusters = L.clusters;
    if (i >= clusters) return;
    const DevParams& P = *d.params;
    const T dt = P.dt;
    T devC = static_cast<T>(P.d_dev_compliance), volC = static_cast<T>(P.d_vol_compliance);
    body_compliances(P, L.first[0] + i, devC, volC);
    const T a_dev = devC / dt / dt, a_vol = volC / dt / dt, c_off = volC / devC;
    const uint32_t sub_base = P.epoch + sub * ncol, stamp = sub_base + k + 1u;
    const bool last_sub = sub + 1u == n_sub;
    const int32_t va = L.slot_vid[static_cast<size_t>(c) * clusters + i], vb = L.slot_vid[static_cast<size_t>(c + 4u) * clusters + i];
    const float ima = C.slot_im[static_cast<size_t>(c) * clusters + i], imb = C.slot_im[static_cast<size_t>(c + 4u) * clusters + i];
    const uint2 dl = C.delta[i], df = C.delta_first[i];
    const uint32_t lmask = C.last_mask[i], fmask = L.first_mask[i];
    uint32_t cs[kNHClusterTets];
    float4 ia[kNHClusterTets], ib[kNHClusterTets], ic[kNHClusterTets];
    int32_t ord[kNHClusterTets];
    auto request = [&](uint32_t j) {
        const uint32_t e = (j < L.nsteps && i < L.count[j]) ? L.first[j] + i : L.first[0] + i;
        cs[j] = d.corner_slots[e];
        ia[j] = d.irp_a[e]; ib[j] = d.irp_b[e]; ic[j] = d.irp_c[e];
        ord[j] = d.order[e];
    };
    request(0);
    __builtin_amdgcn_sched_barrier(0);
    const bool first_a = (fmask >> c) & 1u, first_b = (fmask >> (c + 4u)) & 1u;
    const uint32_t da = ((first_a ? df.x : dl.x) >> (8u * c)) & 0xffu, db = ((first_b ? df.y : dl.y) >> (8u * c)) & 0xffu;
    const uint32_t want_a = stamp - da, want_b = stamp - db;
    const uint32_t ua = va < 0 ? 0u : static_cast<uint32_t>(va), ub = vb < 0 ? 0u : static_cast<uint32_t>(vb);
    // a first touch of the launch's first substep reads NHDev::pos (the prediction kernel in front of this launch wrote it); everything else is handed on
    bool pend_a = va >= 0 && !(first_a && sub == 0u), pend_b = vb >= 0 && !(first_b && sub == 0u);
    const bool fold_a = first_a && sub != 0u && va >= 0, fold_b = first_b && sub != 0u && vb >= 0;
    float4 ga = d.pos[ua], gb = d.pos[ub];
    float4 xa = load_coherent(xch, ua), xb = load_coherent(xch, ub);
    float4 pa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pb = pa;
    if (fold_a) pa = load_coherent(d.prev, ua);
    if (fold_b) pb = load_coherent(d.prev, ub);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (uint32_t j = 1; j < kNHClusterTets; j++) request(j);
    __builtin_amdgcn_sched_barrier(0);
    if (pend_a && __float_as_uint(xa.w) == want_a) { ga = xa; pend_a = false; }
    if (pend_b && __float_as_uint(xb.w) == want_b) { gb = xb; pend_b = false; }
    // (the previous position of a folded particle: this lane's own store of one substep ago, stamped with that substep's base; the
    // prediction kernel's at the launch's second substep; until the awaited store lands the lane holds 0 or an older substep's base, never it)
    bool ppend_a = fold_a && sub > 1u && __float_as_uint(pa.w) != sub_base - ncol, ppend_b = fold_b && sub > 1u && __float_as_uint(pb.w) != sub_base - ncol;
    if (__builtin_amdgcn_ballot_w64(pend_a || pend_b || ppend_a || ppend_b) != 0ull) {
        const long long t0 = wall_clock64(), limit = 100000ll * timeout_ms;   // 100 MHz ticks; 0 = unbounded
        do {
            __builtin_amdgcn_s_sleep(TETSIM_NH_POLL_SLEEP);
            asm volatile("" ::: "memory");   // (every look is a fresh load)
            if (pend_a) { xa = load_coherent(xch, ua); if (__float_as_uint(xa.w) == want_a) { ga = xa; pend_a = false; } }
            if (pend_b) { xb = load_coherent(xch, ub); if (__float_as_uint(xb.w) == want_b) { gb = xb; pend_b = false; } }
            if (ppend_a) { pa = load_coherent(d.prev, ua); ppend_a = __float_as_uint(pa.w) != sub_base - ncol; }
            if (ppend_b) { pb = load_coherent(d.prev, ub); ppend_b = __float_as_uint(pb.w) != sub_base - ncol; }
            if (limit && (pend_a || pend_b || ppend_a || ppend_b) && wall_clock64() - t0 > limit) {
                __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                pend_a = pend_b = ppend_a = ppend_b = false;
            }
        } while (__builtin_amdgcn_ballot_w64(pend_a || pend_b || ppend_a || ppend_b) != 0ull);
    }
    // the particle pass between the two substeps: fold_particle's operations (the velocity array is left to the kernel that ends the call).
    // The position a folded particle had at the end of the substep goes out with the hand-overs at the end of this kernel: its reader is
    // this lane's successor one substep on, and a write-through store issued here is in the way of the first vmcnt(0) behind it -- the
    // solves of colour 0 started ~1 us late (tools/nh_link_trace.py)
    float4 keep_a = pa, keep_b = pb;
    if (fold_a || fold_b) {
        const VParams vp = load_vparams_of(P, cluster_body(P, L.first[0] + i));
        auto fold = [&](uint32_t v, float4& pos, const float4& prev_in, float4& prev) {
            float4 vel;
            post_vertex<false>(vp, v, pos, prev_in, vel);
            predict_vertex(vp, vel, pos, prev);
            prev.w = __uint_as_float(sub_base);
        };
        if (fold_a) fold(ua, ga, pa, keep_a);
        if (fold_b) fold(ub, gb, pb, keep_b);
    }
    ga.w = ima; gb.w = imb;
    s_pos[c * 16u + cl] = ga;
    s_pos[(c + 4u) * 16u + cl] = gb;
    float* const sp = reinterpret_cast<float*>(s_pos);
#pragma unroll
    for (uint32_t j = 0; j < kNHClusterTets; j++) {
        if (j >= L.nsteps) break;            // (uniform)
        if (i < L.count[j]) {
            const uint32_t a0 = ((cs[j] << 6) & 0x3fc0u) + lane, a1 = ((cs[j] >> 2) & 0x3fc0u) + lane,
                           a2 = ((cs[j] >> 10) & 0x3fc0u) + lane, a3 = ((cs[j] >> 18) & 0x3fc0u) + lane;
            float p[4] = {sp[a0], sp[a1], sp[a2], sp[a3]};
            const float im[4] = {quad<kQuadLane3>(p[0]), quad<kQuadLane3>(p[1]), quad<kQuadLane3>(p[2]), quad<kQuadLane3>(p[3])};
            const float ir[9] = {ia[j].x, ia[j].y, ia[j].z, ia[j].w, ib[j].x, ib[j].y, ib[j].z, ib[j].w, ic[j].x};
            const T ve = solve_quad(p, im, ir, static_cast<T>(ic[j].y), a_dev, a_vol, c_off);
            if (c == 0u && d.vol_err && last_sub) d.vol_err[ord[j]] = static_cast<double>(ve);
            if (c < 3u) { sp[a0] = p[0]; sp[a1] = p[1]; sp[a2] = p[2]; sp[a3] = p[3]; }
        }
    }
    // the hand-over of nh_sweep1_kernel, to NHDev::pos in the call's last substep only
    if (va >= 0) {
        float4 r = s_pos[c * 16u + cl];
        if (((lmask >> c) & 1u) && last_sub) store_wt(d.pos, ua, r);
        else { r.w = __uint_as_float(stamp); store_wt(xch, ua, r); }
    }
    if (vb >= 0) {
        float4 r = s_pos[(c + 4u) * 16u + cl];
        if (((lmask >> (c + 4u)) & 1u) && last_sub) store_wt(d.pos, ub, r);
        else { r.w = __uint_as_float(stamp); store_wt(xch, ub, r); }
    }
    if (fold_a) store_wt(d.prev, ua, keep_a);
    if (fold_b) store_wt(d.prev, ub, keep_b);
}
#endif

// the instantiation of a kernel by a launch-time flag: either(wt, either(fold, k<true, true>, k<true, false>), ...)
template <class K>
K* either(bool flag, K* yes, K* no) { return flag ? yes : no; }

}  // namespace

#if TETSIM_FAST
void nh_launch_call_fast(hipStream_t s, const NHDev& d, const NHSweep& w, uint32_t n) {
    if (w.blocks == 0 || n == 0) return;
    const uint32_t per_sub = nh_call_blocks_per_sub(w.blocks);
    hipLaunchKernelGGL(nh_call_kernel, dim3(per_sub * n), dim3(256), 0, s, w.colours, w.ncolours, w.exchange, n, per_sub, w.blocks, w.error, w.timeout_ms, d);
}
void nh_launch_sweep1_fast(hipStream_t s, const NHDev& d, const NHSweep& w, bool fold, uint32_t sub_index, uint32_t epoch) {
    if (w.blocks == 0) return;
    hipLaunchKernelGGL(either(fold, nh_sweep1_kernel<true>, nh_sweep1_kernel<false>), dim3(w.blocks), dim3(256), 0, s, w.colours, w.ncolours, w.exchange, sub_index, epoch, w.error, w.timeout_ms, d);
}
#endif

void TETSIM_SFX(nh_launch_predict_)(hipStream_t s, const NHDev& d) {
    if (d.nv == 0) return;
    hipLaunchKernelGGL(TETSIM_SFX(nh_predict_kernel_), dim3((d.nv + 255u) / 256u), dim3(256), 0, s, d);
}
void TETSIM_SFX(nh_launch_predict_value_)(hipStream_t s, const NHDev& d, const DevParams& params, DevParams* params_dev) {
    if (d.nv == 0) return;
    hipLaunchKernelGGL(TETSIM_SFX(nh_predict_value_kernel_), dim3((d.nv + 255u) / 256u), dim3(256), 0, s, d, params, params_dev);
}
void TETSIM_SFX(nh_launch_level_)(hipStream_t s, const NHDev& d, uint32_t first, uint32_t count) {
    if (count == 0) return;
    // one wave per workgroup unless the level alone fills the chip several times over: a colour of the 1 M-tet lattice is
    // ~32 k tets = 503 waves, which 256-thread workgroups would pack onto half of the 256 CUs
    const uint32_t block = count >= 262144u ? 256u : 64u;
    // write-through stores pay on big levels (1 M-tet lattice, 32 k tets per colour: 191 -> 163 us per substep) and cost 3-5% on
    // the Dragon's 120-tet levels, whose next level finds the lines in the same L2
    hipLaunchKernelGGL(either(count >= 4096u, TETSIM_SFX(nh_level_kernel_)<true>, TETSIM_SFX(nh_level_kernel_)<false>), dim3((count + block - 1u) / block), dim3(block), 0, s, d, first, count);
}
void TETSIM_SFX(nh_launch_level4_)(hipStream_t s, const NHDev& d, uint32_t first, uint32_t count) {
    if (count == 0) return;
    hipLaunchKernelGGL(TETSIM_SFX(nh_level4_kernel_), dim3((count + 63u) / 64u), dim3(256), 0, s, d, first, count);
}
void TETSIM_SFX(nh_launch_cluster_)(hipStream_t s, const NHDev& d, const NHClusterLaunch& L, bool fold) {
    if (L.clusters == 0) return;
    fold = fold && L.first_mask != nullptr;
    const bool wt = L.clusters >= 1024u;   // small launches: see nh_launch_level_
#if TETSIM_FAST
#ifdef TETSIM_ABLATION
    static const bool quads = [] { const char* e = getenv("TETSIM_NH_QUADS"); return !(e && e[0] == '0'); }();   // (development build, =0: one lane per cluster, A/B)
#else
    constexpr bool quads = true;
#endif
#else
    // PRECISE on four lanes gives the same bits (solve_quad adds every sum up in the reference's order in every lane) and a shorter
    // chain, but four times the f64 work: it pays while a launch is a few waves -- the Dragon's 11 cluster colours 149 -> 103 us per
    // substep -- and loses once the launch fills the chip (1 M-tet lattice: 130.6 against 119.8 us).
    const bool quads = L.clusters <= 2048u;
#endif
    if (quads) {
        const dim3 grid((L.clusters + 63u) / 64u), block(256);
        const float4* cpos = d.pos;
        const float4* cprev = d.prev;
        auto* kernel = either(wt, either(fold, TETSIM_SFX(nh_cluster4_kernel_)<true, true>, TETSIM_SFX(nh_cluster4_kernel_)<true, false>),
                              either(fold, TETSIM_SFX(nh_cluster4_kernel_)<false, true>, TETSIM_SFX(nh_cluster4_kernel_)<false, false>));
        hipLaunchKernelGGL(kernel, grid, block, 0, s, L.slot_vid, cpos, L.first_mask, cprev, L.clusters, d, L);
        return;
    }
    auto* kernel = either(wt, either(fold, TETSIM_SFX(nh_cluster_kernel_)<true, true>, TETSIM_SFX(nh_cluster_kernel_)<true, false>),
                          either(fold, TETSIM_SFX(nh_cluster_kernel_)<false, true>, TETSIM_SFX(nh_cluster_kernel_)<false, false>));
    hipLaunchKernelGGL(kernel, dim3((L.clusters + 63u) / 64u), dim3(64), 0, s, d, L);
}
uint32_t TETSIM_SFX(nh_frame_lds_limit_)() {
    // (a kernel may use all of a CU's LDS once it says so -- per device: asked for at every create, on the body's device)
    const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(TETSIM_SFX(nh_frame_kernel_)), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok ? 160u * 1024u : 64u * 1024u;
}
void TETSIM_SFX(nh_launch_frame_)(hipStream_t s, const NHDev& d, const NHFrameLaunch& f, uint32_t n, const DevParams& params, DevParams* params_dev) {
    if (d.nv == 0 || n == 0 || f.bodies == 0) return;
    hipLaunchKernelGGL(TETSIM_SFX(nh_frame_kernel_), dim3(f.bodies), dim3(f.block), f.max_body_particles * 40u, s, d, f.seg, f.first_vert, f.levels, f.bodies, n, params, params_dev);
}
void TETSIM_SFX(nh_launch_post_predict_list_)(hipStream_t s, const NHDev& d, const uint32_t* list, uint32_t n) {
    if (n == 0) return;
    hipLaunchKernelGGL(TETSIM_SFX(nh_post_predict_list_kernel_), dim3((n + 255u) / 256u), dim3(256), 0, s, d, list, n);
}
void TETSIM_SFX(nh_launch_post_)(hipStream_t s, const NHDev& d) {
    if (d.nv == 0) return;
    hipLaunchKernelGGL(TETSIM_SFX(nh_post_kernel_), dim3((d.nv + 255u) / 256u), dim3(256), 0, s, d);
}
void TETSIM_SFX(nh_launch_post_predict_)(hipStream_t s, const NHDev& d) {
    if (d.nv == 0) return;
    hipLaunchKernelGGL(TETSIM_SFX(nh_post_predict_kernel_), dim3((d.nv + 255u) / 256u), dim3(256), 0, s, d);
}
// this mode's instance of the launcher table (dev_common.h); host pass only: a const object would be emitted for the device too, where no launcher exists
#if !defined(__HIP_DEVICE_COMPILE__)
const NHLaunchers TETSIM_SFX(nh_launchers_) = {
    TETSIM_SFX(nh_launch_predict_), TETSIM_SFX(nh_launch_predict_value_), TETSIM_SFX(nh_launch_level_), TETSIM_SFX(nh_launch_level4_), TETSIM_SFX(nh_launch_cluster_),
    TETSIM_SFX(nh_launch_post_), TETSIM_SFX(nh_launch_post_predict_), TETSIM_SFX(nh_launch_post_predict_list_), TETSIM_SFX(nh_launch_frame_), TETSIM_SFX(nh_frame_lds_limit_)};
#endif

}  // namespace tetsim
