// pj_kernels.inc -- POLAR_JACOBI substep kernels for gfx950 (wave64), included by pj_precise.hip
// (-ffp-contract=off) and pj_fast.hip with TETSIM_FAST = 0 / 1.
//
// One substep of the reference's WebGL solver is 7 full-screen passes (SoftbodyGPU.js:59-376):
//   P1 prev=pos  P2 pos+=vel*dt  P3 rotation extraction  P4 goal positions  P5 weighted average
//   P6 grab/clamp/floor  P7 velocity.
// Here it is TWO kernels over double-role device arrays (no ping-pong copies are needed because every
// thread reads and writes only its own element of the arrays it updates):
//   pj_tet_kernel    = P3 + P4   one lane per tet: gathers the 4 predicted corner positions, extracts the
//                                rotation, writes quat and the 4 goal corners (xyz, w = rest volume).
//   pj_vertex_kernel = P5 + P6 + P7 of substep n, then P1 + P2 of substep n+1, one lane per particle:
//                                gathers its incident goals in the reference's slot order, averages,
//                                collides, derives the velocity and stores x_final, v and the next
//                                prediction x* = x_final + v*dt.
// The arithmetic inside each lane is written in the order of the GLSL source so that the PRECISE build
// (IEEE f32, no contraction) differs from the CPU restatement only through sin().
#include "collide.h"
#include "dev_common.h"
#include "pj_lab.h"

// kernels and launchers carry the arithmetic mode in their names (pj_tet_kernel_precise / _fast ...)
#define TETSIM_CAT_(a, b) a##b
#define TETSIM_CAT(a, b) TETSIM_CAT_(a, b)
#define TETSIM_SFX(name) TETSIM_CAT(name, TETSIM_MODE_SUFFIX)

namespace tetsim {
namespace {

#include "pj_math.inc"

// Workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8, each with a private 4 MiB
// L2).  Remap so that every XCD walks ONE contiguous eighth of the tiles: its L2 then holds an eighth of
// the vertex array (plus a halo) instead of all of it.  Purely a locality choice; any placement is correct.
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t tiles_per_xcd) {
    return (b & 7u) * tiles_per_xcd + (b >> 3);
}

// ---------------------------------------------------------------------------------------------------
// P3 + P4
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void TETSIM_SFX(pj_tet_kernel_)(PJDev d, uint32_t tiles, uint32_t tiles_per_xcd) {
    const uint32_t tile = xcd_tile(blockIdx.x, tiles_per_xcd);
    const uint32_t e = tile * 256u + threadIdx.x;
    if (tile >= tiles || e >= d.nt) return;

    const int4 id = d.tet_idx[e];
    float4 r4[4];
#pragma unroll
    for (int k = 0; k < 4; k++) r4[k] = d.elem[static_cast<size_t>(k) * d.nt_pad + e];
    const float4 q_old = d.quat[e];
    f3 cur[4];
    cur[0] = xyz(d.pos_pred[id.x]);
    cur[1] = xyz(d.pos_pred[id.y]);
    cur[2] = xyz(d.pos_pred[id.z]);
    cur[3] = xyz(d.pos_pred[id.w]);
    f3 rest[4];
#pragma unroll
    for (int k = 0; k < 4; k++) rest[k] = xyz(r4[k]);

    float4 q_new;
    f3 goal[4];
    pj_solve_tet(cur, rest, q_old, q_new, goal, 9, true, false, false, nullptr, d.rot_exit_w2);
    d.quat[e] = q_new;
#pragma unroll
    for (int k = 0; k < 4; k++)
        d.elem[static_cast<size_t>(k) * d.nt_pad + e] = make_float4(goal[k].x, goal[k].y, goal[k].z, r4[k].w);
}
// ---------------------------------------------------------------------------------------------------
// P5 + P6 + P7 (+ P1, P2 of the next substep)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void TETSIM_SFX(pj_vertex_kernel_)(PJDev d, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t v = first + i;
    const DevParams& P = *d.params;

    // P5, SoftbodyGPU.js:302-320: volume-weighted mean of the incident goal corners, in slot order.
    // The loop is latency bound if taken one slot at a time (index load -> dependent 16-byte gather, ~23 deep
    // per particle), so 8 slots are fetched together -- 8 independent gathers in flight per lane -- and then
    // accumulated strictly in slot order (the order is part of the result in f32).
    const uint32_t cnt = d.slot_cnt[v];
    const float4 prev4 = d.pos_final[v];  // requested up front: behind the slot loop it would be one more memory round trip
    f3 sum = F3(0.0f, 0.0f, 0.0f);
    float wsum = 0.0f;
    const int32_t* col = d.slot_tab + v;
    for (uint32_t s0 = 0; s0 < cnt; s0 += 8u) {
        int32_t idx[8];
        float4 ev[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) idx[j] = (s0 + j < cnt) ? col[static_cast<size_t>(s0 + j) * d.nv_pad] : -1;
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) ev[j] = idx[j] >= 0 ? d.elem[idx[j]] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++)
            if (s0 + j < cnt) {
                sum = sum + xyz(ev[j]) * ev[j].w;
                wsum += ev[j].w;
            }
    }
    f3 p;
    if constexpr (kFast) { const float r = __builtin_amdgcn_rcpf(wsum); p = sum * r; }
    else p = F3(sum.x / wsum, sum.y / wsum, sum.z / wsum);  // 0/0 = NaN for a particle with no tets, as in the reference

    // P6, :340-355
    const f3 prev = xyz(prev4);  // end of the previous substep == texturePrevPos after P1
    bool grabbed = static_cast<int32_t>(v) == P.grab_local || static_cast<int32_t>(v) == P.grab_local2;
    if (grabbed) p = F3(P.grab[0], P.grab[1], P.grab[2]);
    body_grab_pick(P, v, grabbed, p.x, p.y, p.z);   // (body grabs, dev_common.h: a selection behind one uniform branch, no arithmetic)
    const PolarBodyParams B = body_params_polar<false>(P, v);   // (body parameters, dev_common.h: the call's values or, per lane, the body's row)
    p.x = fminf(fmaxf(p.x, B.lo[0]), B.hi[0]);
    p.y = fminf(fmaxf(p.y, B.lo[1]), B.hi[1]);
    p.z = fminf(fmaxf(p.z, B.lo[2]), B.hi[2]);
    if (p.y < 0.0f) {
        p.y = 0.0f;
        const f3 F = prev - p;
        const float fr = fminf(1.0f, P.dt * B.friction);
        p.x += F.x * fr;
        p.z += F.z * fr;
    }
    if (any_colliders(P)) collide_particle_f32<kFast>(p.x, p.y, p.z, prev.x, prev.y, prev.z, P, v, !grabbed);   // kinematic colliders (collide.h): the handle's list or the body's
    // P7, :364-372
    const f3 dpos = p - prev;
    f3 vel;
    if constexpr (kFast) { const float r = __builtin_amdgcn_rcpf(P.dt); vel = dpos * r; }
    else vel = F3(dpos.x / P.dt, dpos.y / P.dt, dpos.z / P.dt);
    vel = vel + F3(0.0f, B.gravity, 0.0f) * P.dt;

    d.pos_final[v] = make_float4(p.x, p.y, p.z, 0.0f);
    d.vel[v] = make_float4(vel.x, vel.y, vel.z, 0.0f);
    // next substep's P1 (prev = pos: that is pos_final) and P2 (:67-74)
    const f3 pred = p + vel * P.dt;
    d.pos_pred[v] = make_float4(pred.x, pred.y, pred.z, 0.0f);
}

// x* = x + v*dt again, when the caller changes dt between substeps (the fused prediction used the old dt)
__global__ __launch_bounds__(256) void TETSIM_SFX(pj_repredict_kernel_)(PJDev d) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= d.nv_owned) return;
    const float dt = d.params->dt;
    const f3 pred = xyz(d.pos_final[v]) + xyz(d.vel[v]) * dt;
    d.pos_pred[v] = make_float4(pred.x, pred.y, pred.z, 0.0f);
}

}  // namespace


void TETSIM_SFX(pj_launch_tet_)(hipStream_t s, const PJDev& d, hipEvent_t e0, hipEvent_t e1) {
    if (d.nt == 0) return;
    const uint32_t tiles = (d.nt + 255u) / 256u;
    const uint32_t per_xcd = (tiles + 7u) / 8u;
    if (e0) hipExtLaunchKernelGGL(TETSIM_SFX(pj_tet_kernel_), dim3(per_xcd * 8u), dim3(256), 0, s, e0, e1, 0, d, tiles, per_xcd);
    else hipLaunchKernelGGL(TETSIM_SFX(pj_tet_kernel_), dim3(per_xcd * 8u), dim3(256), 0, s, d, tiles, per_xcd);
}
void TETSIM_SFX(pj_launch_vertex_)(hipStream_t s, const PJDev& d, uint32_t first, uint32_t count, hipEvent_t e0, hipEvent_t e1) {
    if (count == 0) return;
    if (e0) hipExtLaunchKernelGGL(TETSIM_SFX(pj_vertex_kernel_), dim3((count + 255u) / 256u), dim3(256), 0, s, e0, e1, 0, d, first, count);
    else hipLaunchKernelGGL(TETSIM_SFX(pj_vertex_kernel_), dim3((count + 255u) / 256u), dim3(256), 0, s, d, first, count);
}
void TETSIM_SFX(pj_launch_repredict_)(hipStream_t s, const PJDev& d) {
    if (d.nv_owned == 0) return;
    hipLaunchKernelGGL(TETSIM_SFX(pj_repredict_kernel_), dim3((d.nv_owned + 255u) / 256u), dim3(256), 0, s, d);
}
// this mode's instance of the launcher table (dev_common.h); host pass only: a const object would be emitted for the device too, where no launcher exists
#if !defined(__HIP_DEVICE_COMPILE__)
const PJLaunchers TETSIM_SFX(pj_launchers_) = {TETSIM_SFX(pj_launch_tet_), TETSIM_SFX(pj_launch_vertex_), TETSIM_SFX(pj_launch_repredict_)};
#endif

}  // namespace tetsim
