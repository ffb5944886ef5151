// place.hip -- C ABI, part 7 (include/tetsim.h): tetsim_place_bodies / _device.  One rigid motion per CHOSEN body of a batch, applied to the
// complete solver state -- every section state_sections() lists (tetsim_state.hip): positions, velocities, the polar solver's predictions,
// quaternions and carried shapes, the Neo-Hookean previous positions -- by ONE kernel on the handle's stream, ordered against the caller's
// stream as the device import is (body.h: on_caller_stream).  Rows and mask are device memory that the host never reads; a row finds its
// body through the snapshots' tables (snapshot.hip: ensure_body_tables).  Built with -ffp-contract=off: the definition in the header is f64 with
// every operation rounded on its own, and tests/place_ref.py reproduces it value for value in numpy.  See body.h.
#include "body_rows.h"

using namespace tetsim;

namespace tetsim {
namespace {

// how a polar body carries its shape (state_sections: which arrays; pj_math.inc: pj_solve_tet, what they mean)
enum : uint32_t {
    kShapeNone = 0u,       // Neo-Hookean; constant-rest-shape bodies
    kShapeCentred12 = 1u,  // blocked: rest_a / rest_b / rest_c, four corners relative to their own centroid
    kShapeCentred9 = 2u,   // TETSIM_FLAG_LEAN_STATE: rest_a / rest_b / rest_c1, three such corners
    kShapePlanes = 3u,     // gather formulation: elem [4][nt_pad], world-space corners in xyz (w: the rest volume)
};
struct PlaceTable {
    float4 *pos, *vel;
    float4* pred;                  // polar: the predictions, left as pos' + vel' * dt; else null
    float4* prev;                  // Neo-Hookean: the previous positions, placed as positions are; else null
    float4* quat;                  // polar: [nt]; else null
    float4 *shape_a, *shape_b, *shape_c;   // kShapeCentred12 / 9: the records; kShapePlanes: shape_a = elem
    float* shape_c1;
    const uint32_t *first_vert, *first_elem;   // [bodies + 1] first row of every body, device numbering
    const char* rows;              // body b's row of TETSIM_PLACE_WIDTH floats at rows + b * stride
    uint64_t stride;
    const uint8_t* mask;           // [bodies] nonzero = chosen; null = all
    uint32_t nv, nt, nt_pad, shape;
    uint32_t bodies, keep_velocity;
    uint32_t tet_first_block;      // the grid: particle chunks, then tet chunks
    float dt;                      // of the predictions (0 while they are stale or valid for any dt: the next step predicts afresh)
};
static_assert(sizeof(PlaceTable) <= 512, "the table is a kernel argument");

constexpr uint32_t kPlaceLanes = 256;   // a workgroup = a chunk of 256 rows, one row per lane
constexpr uint32_t kPlaceSpan = 8;      // bodies of a chunk whose motion the workgroup works out once (a chunk of smaller bodies: every lane its own)

// the motion of one body, worked out from its row
struct Motion {
    double m[3][3];
    double pivot[3], centre[3], linear[3], angular[3];
    double q[4];                   // the unit quaternion, xyzw
    uint32_t valid;                // chosen, every float finite, |q| != 0
};

__device__ __forceinline__ uint32_t body_of_row(const uint32_t* __restrict__ first, uint32_t bodies, uint32_t row) {
    if (row >= first[bodies]) return bodies;   // padding
    uint32_t lo = 0, hi = bodies;              // first[lo] <= row < first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ void make_motion(const PlaceTable& t, uint32_t b, Motion& M) {
    M.valid = 0u;
    if (t.mask && t.mask[b] == 0) return;
    const float* const r = reinterpret_cast<const float*>(t.rows + static_cast<uint64_t>(b) * t.stride);
    float f[TETSIM_PLACE_WIDTH];
    bool ok = true;
#pragma unroll
    for (uint32_t i = 0; i < TETSIM_PLACE_WIDTH; i++) { f[i] = r[i]; ok = ok && finite_f32(f[i]); }
    if (!ok) return;
    const double qx = f[TETSIM_PLACE_Q], qy = f[TETSIM_PLACE_Q + 1], qz = f[TETSIM_PLACE_Q + 2], qw = f[TETSIM_PLACE_Q + 3];
    const double n = sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw);
    if (n == 0.0) return;
    const double x = qx / n, y = qy / n, z = qz / n, w = qw / n;
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    M.m[0][0] = 1.0 - 2.0 * (yy + zz); M.m[0][1] = 2.0 * (xy - wz);       M.m[0][2] = 2.0 * (xz + wy);
    M.m[1][0] = 2.0 * (xy + wz);       M.m[1][1] = 1.0 - 2.0 * (xx + zz); M.m[1][2] = 2.0 * (yz - wx);
    M.m[2][0] = 2.0 * (xz - wy);       M.m[2][1] = 2.0 * (yz + wx);       M.m[2][2] = 1.0 - 2.0 * (xx + yy);
    M.q[0] = x; M.q[1] = y; M.q[2] = z; M.q[3] = w;
#pragma unroll
    for (uint32_t i = 0; i < 3u; i++) {
        M.pivot[i] = f[TETSIM_PLACE_PIVOT + i];
        M.centre[i] = M.pivot[i] + static_cast<double>(f[TETSIM_PLACE_OFFSET + i]);
        M.linear[i] = f[TETSIM_PLACE_LINEAR + i];
        M.angular[i] = f[TETSIM_PLACE_ANGULAR + i];
    }
    M.valid = 1u;
}

struct d3 { double x, y, z; };
__device__ __forceinline__ d3 rot(const Motion& M, double dx, double dy, double dz) {
    return {(M.m[0][0] * dx + M.m[0][1] * dy) + M.m[0][2] * dz, (M.m[1][0] * dx + M.m[1][1] * dy) + M.m[1][2] * dz,
            (M.m[2][0] * dx + M.m[2][1] * dy) + M.m[2][2] * dz};
}
// a world-space point: Rot(e - pivot) + centre, before the rounding to f32
__device__ __forceinline__ d3 place_point(const Motion& M, float ex, float ey, float ez) {
    const d3 r = rot(M, static_cast<double>(ex) - M.pivot[0], static_cast<double>(ey) - M.pivot[1], static_cast<double>(ez) - M.pivot[2]);
    return {r.x + M.centre[0], r.y + M.centre[1], r.z + M.centre[2]};
}

__device__ __forceinline__ void place_particle(const PlaceTable& t, const Motion& M, uint32_t v) {
    const float4 p = t.pos[v], u4 = t.vel[v];
    const d3 r = rot(M, static_cast<double>(p.x) - M.pivot[0], static_cast<double>(p.y) - M.pivot[1], static_cast<double>(p.z) - M.pivot[2]);
    const float4 pn = make_float4(static_cast<float>(r.x + M.centre[0]), static_cast<float>(r.y + M.centre[1]), static_cast<float>(r.z + M.centre[2]), p.w);
    // u = linear + cross(angular, r)
    d3 u = {M.linear[0] + (M.angular[1] * r.z - M.angular[2] * r.y), M.linear[1] + (M.angular[2] * r.x - M.angular[0] * r.z),
            M.linear[2] + (M.angular[0] * r.y - M.angular[1] * r.x)};
    if (t.keep_velocity) {
        const d3 rv = rot(M, u4.x, u4.y, u4.z);
        u = {rv.x + u.x, rv.y + u.y, rv.z + u.z};
    }
    const float4 vn = make_float4(static_cast<float>(u.x), static_cast<float>(u.y), static_cast<float>(u.z), u4.w);
    t.pos[v] = pn;
    t.vel[v] = vn;
    if (t.pred) {   // the re-prediction kernel's arithmetic (pj_kernels.inc): a product, then a sum, in f32
        const float w = t.pred[v].w;
        const float ax = vn.x * t.dt, ay = vn.y * t.dt, az = vn.z * t.dt;
        t.pred[v] = make_float4(pn.x + ax, pn.y + ay, pn.z + az, w);
    }
    if (t.prev) {
        const float4 o = t.prev[v];
        const d3 e = place_point(M, o.x, o.y, o.z);
        t.prev[v] = make_float4(static_cast<float>(e.x), static_cast<float>(e.y), static_cast<float>(e.z), o.w);
    }
}

__device__ __forceinline__ void place_tet(const PlaceTable& t, const Motion& M, uint32_t e) {
    if (t.quat && e < t.nt) {   // q' = qR (x) q in the reference's term order (SoftbodyGPU.js:114-121), not renormalised
        const float4 q = t.quat[e];
        const double ax = M.q[0], ay = M.q[1], az = M.q[2], aw = M.q[3];
        const double bx = q.x, by = q.y, bz = q.z, bw = q.w;
        t.quat[e] = make_float4(static_cast<float>(((aw * bx + ax * bw) + ay * bz) - az * by), static_cast<float>(((aw * by - ax * bz) + ay * bw) + az * bx),
                                static_cast<float>(((aw * bz + ax * by) - ay * bx) + az * bw), static_cast<float>(((aw * bw - ax * bx) - ay * by) - az * bz));
    }
    if (t.shape == kShapePlanes) {
#pragma unroll
        for (uint32_t c = 0; c < 4u; c++) {
            float4* const at = t.shape_a + static_cast<size_t>(c) * t.nt_pad + e;
            const float4 o = *at;
            const d3 n = place_point(M, o.x, o.y, o.z);
            *at = make_float4(static_cast<float>(n.x), static_cast<float>(n.y), static_cast<float>(n.z), o.w);
        }
    } else if (t.shape == kShapeCentred12 || t.shape == kShapeCentred9) {   // corner k's component c is float 3k + c of the record (dev_common.h: PJBlk)
        const float4 a = t.shape_a[e], b = t.shape_b[e];
        const d3 r0 = rot(M, a.x, a.y, a.z), r1 = rot(M, a.w, b.x, b.y);
        t.shape_a[e] = make_float4(static_cast<float>(r0.x), static_cast<float>(r0.y), static_cast<float>(r0.z), static_cast<float>(r1.x));
        if (t.shape == kShapeCentred9) {
            const d3 r2 = rot(M, b.z, b.w, t.shape_c1[e]);
            t.shape_b[e] = make_float4(static_cast<float>(r1.y), static_cast<float>(r1.z), static_cast<float>(r2.x), static_cast<float>(r2.y));
            t.shape_c1[e] = static_cast<float>(r2.z);
        } else {
            const float4 c = t.shape_c[e];
            const d3 r2 = rot(M, b.z, b.w, c.x), r3 = rot(M, c.y, c.z, c.w);
            t.shape_b[e] = make_float4(static_cast<float>(r1.y), static_cast<float>(r1.z), static_cast<float>(r2.x), static_cast<float>(r2.y));
            t.shape_c[e] = make_float4(static_cast<float>(r2.z), static_cast<float>(r3.x), static_cast<float>(r3.y), static_cast<float>(r3.z));
        }
    }
}

// A workgroup = 256 consecutive rows of the particles or of the tets, a lane = one row with everything the state holds of it: 16-byte loads
// and stores, consecutive lanes on consecutive rows.  The bodies the chunk spans (one, unless a boundary falls inside it) get their motion
// worked out once, by the workgroup's first lanes, into LDS; a chunk none of whose bodies is placed has read mask bytes only.
__global__ __launch_bounds__(kPlaceLanes) void place_kernel(PlaceTable t) {
    __shared__ Motion s_motion[kPlaceSpan];
    const bool tets = blockIdx.x >= t.tet_first_block;                       // (uniform)
    const uint32_t* const first = tets ? t.first_elem : t.first_vert;
    const uint32_t n = tets ? (t.shape == kShapePlanes ? t.nt_pad : t.nt) : t.nv;
    const uint32_t r0 = (blockIdx.x - (tets ? t.tet_first_block : 0u)) * kPlaceLanes;
    if (r0 >= n) return;
    const uint32_t r1 = (r0 + kPlaceLanes < n ? r0 + kPlaceLanes : n) - 1u;  // the chunk's last row
    const uint32_t b0 = body_of_row(first, t.bodies, r0);
    if (b0 == t.bodies) return;                                              // padding only
    uint32_t b1 = body_of_row(first, t.bodies, r1);
    if (b1 == t.bodies) b1 = t.bodies - 1u;
    const uint32_t span = b1 - b0 + 1u < kPlaceSpan ? b1 - b0 + 1u : kPlaceSpan;
    if (threadIdx.x < span) make_motion(t, b0 + threadIdx.x, s_motion[threadIdx.x]);
    __syncthreads();
    const uint32_t row = r0 + threadIdx.x;
    if (row > r1) return;
    const uint32_t b = b0 == b1 ? b0 : body_of_row(first, t.bodies, row);
    if (b >= t.bodies) return;
    Motion M = s_motion[b - b0 < kPlaceSpan ? b - b0 : 0u];
    if (b - b0 >= kPlaceSpan) make_motion(t, b, M);
    if (!M.valid) return;
    if (tets) place_tet(t, M, row); else place_particle(t, M, row);
}

// the host variant's rows and mask travel as kernel arguments, a chunk per launch, into a table of the handle's
constexpr uint32_t kRowsPerLaunch = 32;
struct PlaceChunk { float row[kRowsPerLaunch][TETSIM_PLACE_WIDTH]; uint8_t mask[kRowsPerLaunch]; };
static_assert(sizeof(PlaceChunk) + 64 <= kKernelArgLimit, "a chunk of rows is a kernel argument");
__global__ __launch_bounds__(kRowsPerLaunch * TETSIM_PLACE_WIDTH) void place_rows_value_kernel(PlaceChunk c, float* __restrict__ rows, uint8_t* __restrict__ mask, uint32_t first, uint32_t count) {
    const uint32_t i = threadIdx.x / TETSIM_PLACE_WIDTH, k = threadIdx.x % TETSIM_PLACE_WIDTH;
    if (i >= count) return;
    rows[static_cast<size_t>(first + i) * TETSIM_PLACE_WIDTH + k] = c.row[i][k];
    if (k == 0u) mask[first + i] = c.mask[i];
}

// every section of the state is one this file knows how to move (or the Neo-Hookean volError, which a rigid motion leaves alone): a new
// state array must be given its rule here before a placement may run
int check_sections(tetsim_body* h, const PlaceTable& t) {
    std::vector<StateSection> secs;
    state_sections(h, secs);
    for (const StateSection& sec : secs) {
        if (sec.of == StateRows::kSolveOrder) continue;
        const void* p = sec.ptr;
        bool known = p == t.pos || p == t.vel || p == t.pred || p == t.prev || p == t.quat;
        if (t.shape == kShapePlanes) for (uint32_t c = 0; c < 4u; c++) known = known || p == t.shape_a + static_cast<size_t>(c) * t.nt_pad;
        if (t.shape == kShapeCentred12) known = known || p == t.shape_a || p == t.shape_b || p == t.shape_c;
        if (t.shape == kShapeCentred9) known = known || p == t.shape_a || p == t.shape_b || p == t.shape_c1;
        if (!known) return fail(h, TETSIM_ESTATE, "the state holds a section that tetsim_place_bodies has no rule for (place.hip)");
    }
    return 0;
}

PlaceTable make_table(tetsim_body* h, const void* rows, uint64_t stride, const void* mask, uint32_t flags) {
    PlaceTable t{};
    if (h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI) {
        t.pos = h->pj.pos_final; t.vel = h->pj.vel; t.pred = h->pj.pos_pred; t.quat = h->pj.quat;
        t.nv = h->pj.nv_local; t.nt = h->pj.nt; t.nt_pad = h->pj.nt_pad;
        if (!h->blocked) { t.shape = kShapePlanes; t.shape_a = h->pj.elem; }
        else if (h->blk.lean_state) { t.shape = kShapeCentred9; t.shape_a = h->blk.rest_a; t.shape_b = h->blk.rest_b; t.shape_c1 = h->blk.rest_c1; }
        else if (!h->blk.lean) { t.shape = kShapeCentred12; t.shape_a = h->blk.rest_a; t.shape_b = h->blk.rest_b; t.shape_c = h->blk.rest_c; }
    } else {
        t.pos = h->nh.pos; t.vel = h->nh.vel; t.prev = h->nh.prev;
        t.nv = h->nh.nv;
    }
    t.rows = static_cast<const char*>(rows); t.stride = stride; t.mask = static_cast<const uint8_t*>(mask);
    t.bodies = h->info.num_bodies;
    t.keep_velocity = (flags & TETSIM_PLACE_KEEP_VELOCITY) ? 1u : 0u;
    return t;
}

// what either call does once its arguments are good: the tables (the only part that may block), then on h->stream the recovery of a
// lean-state body's quaternions and the one launch
int place(tetsim_body* h, PlaceTable& t, void* caller_stream, bool ordered) {
    if (int rc = ensure_snapshot_body_tables(h)) return rc;
    t.first_vert = h->d_snap_first_vert; t.first_elem = h->d_snap_first_elem;
    auto enqueue = [&]() -> int {
        if (int rc = ensure_quats(h)) return rc;   // (a lean-state body: shape and quaternion turn together, so the recovery's sign rule sees a consistent pair)
        const bool polar = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI;
        // predictions valid for any dt (no substep yet) or stale already: the next step predicts every particle afresh, whatever is left here
        const bool fixed_dt = polar && !h->pred_any_dt && h->dt_pred == h->dt_pred;
        t.dt = fixed_dt ? h->dt_pred : 0.0f;
        const uint32_t tet_rows = polar ? (t.shape == kShapePlanes ? t.nt_pad : t.nt) : 0u;
        t.tet_first_block = (t.nv + kPlaceLanes - 1u) / kPlaceLanes;
        const uint32_t blocks = t.tet_first_block + (tet_rows + kPlaceLanes - 1u) / kPlaceLanes;
        if (blocks) hipLaunchKernelGGL(place_kernel, dim3(blocks), dim3(kPlaceLanes), 0, h->stream, t);
        if (int rc = launched(h)) return rc;
        if (polar && h->pred_any_dt) { h->pred_any_dt = false; h->dt_pred = std::nanf(""); }   // (velocities are no longer zero)
        return 0;
    };
    return ordered ? on_caller_stream(h, caller_stream, enqueue) : enqueue();
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_place_bodies_device(tetsim_handle h, const void* rows, uint64_t row_stride, const void* body_mask, uint32_t flags, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!rows) return fail(h, TETSIM_EINVAL, "rows is null");
    if (flags & ~static_cast<uint32_t>(TETSIM_PLACE_KEEP_VELOCITY)) return fail(h, TETSIM_EINVAL, "unknown flag bits (TETSIM_PLACE_KEEP_VELOCITY is the only one)");
    constexpr uint64_t kRowBytes = 4ull * TETSIM_PLACE_WIDTH;
    if (int rc = check_record_stride(h, "row_stride", row_stride, kRowBytes, 4u)) return rc;
    if (int rc = device_call_guard(h)) return rc;
    const uint32_t nb = h->info.num_bodies;
    const uint64_t stride = resolved_stride(row_stride, kRowBytes);
    if (int rc = check_device_records(h, rows, stride, nb, kRowBytes, 4u, "rows")) return rc;
    if (int rc = check_body_mask(h, body_mask, nb)) return rc;
    PlaceTable t = make_table(h, rows, stride, body_mask, flags);
    if (int rc = check_sections(h, t)) return rc;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    return place(h, t, caller_stream, true);
}

int tetsim_place_bodies(tetsim_handle h, const float* rows, const uint8_t* body_mask, uint32_t flags) {
    if (!h) return TETSIM_EINVAL;
    if (!rows) return fail(h, TETSIM_EINVAL, "rows is null");
    if (flags & ~static_cast<uint32_t>(TETSIM_PLACE_KEEP_VELOCITY)) return fail(h, TETSIM_EINVAL, "unknown flag bits (TETSIM_PLACE_KEEP_VELOCITY is the only one)");
    if (int rc = device_call_guard(h)) return rc;
    const uint32_t nb = h->info.num_bodies;
    for (uint32_t b = 0; b < nb; b++) {
        if (body_mask && body_mask[b] == 0) continue;
        const float* r = rows + static_cast<size_t>(b) * TETSIM_PLACE_WIDTH;
        const std::string at = "body " + std::to_string(b) + ": ";
        for (uint32_t i = 0; i < TETSIM_PLACE_WIDTH; i++)
            if (!std::isfinite(r[i])) return fail(h, TETSIM_EINVAL, at + "non-finite value in its row");
        const double qx = r[TETSIM_PLACE_Q], qy = r[TETSIM_PLACE_Q + 1], qz = r[TETSIM_PLACE_Q + 2], qw = r[TETSIM_PLACE_Q + 3];
        if (std::sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw) == 0.0) return fail(h, TETSIM_EINVAL, at + "zero quaternion");
    }
    if (!h->d_place_rows) {   // (the first call: allocates, so it may block)
        if (int rc = dev_alloc(h, &h->d_place_mask, nb)) return rc;
        if (int rc = dev_alloc(h, &h->d_place_rows, static_cast<size_t>(nb) * TETSIM_PLACE_WIDTH)) return rc;
    }
    PlaceTable t = make_table(h, h->d_place_rows, 4ull * TETSIM_PLACE_WIDTH, h->d_place_mask, flags);
    if (int rc = check_sections(h, t)) return rc;
    // ---- every argument is good
    if (int rc = ensure_snapshot_body_tables(h)) return rc;
    for (uint32_t f = 0; f < nb; f += kRowsPerLaunch) {
        const uint32_t count = std::min(kRowsPerLaunch, nb - f);
        PlaceChunk c{};
        std::memcpy(c.row, rows + static_cast<size_t>(f) * TETSIM_PLACE_WIDTH, static_cast<size_t>(count) * TETSIM_PLACE_WIDTH * sizeof(float));
        for (uint32_t i = 0; i < count; i++) c.mask[i] = body_mask ? (body_mask[f + i] != 0 ? 1u : 0u) : 1u;
        hipLaunchKernelGGL(place_rows_value_kernel, dim3(1), dim3(kRowsPerLaunch * TETSIM_PLACE_WIDTH), 0, h->stream, c, h->d_place_rows, h->d_place_mask, f, count);
    }
    if (int rc = launched(h)) return rc;
    return place(h, t, nullptr, false);
}

}  // extern "C"
