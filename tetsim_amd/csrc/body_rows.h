// body_rows.h -- what the per-body tables share (body_grabs.hip, body_colliders.hip, body_params.hip; place.hip and snapshot.hip use the
// checks).  The public header's promise for them -- a body of a batch, set from device memory, steps bit for bit as it would alone with
// the handle-wide call -- rests on ONE routine per kind of row, compiled for both sides:
//   collider_view / collider_f32   a collider's f64 fields -> the two views the kernels read.  tetsim_set_colliders (tetsim_visual.hip) calls
//                                  it per collider, body_colliders.hip per row of 24 floats (every f32 is exactly a double).
//   params_views                   ten doubles -> the two views of a row of parameters.  fill_params (tetsim_api.hip) takes the call's f32
//                                  values from it, body_params.hip every row's.
// Every unit that includes this is built with -ffp-contract=off: the normalisation rounds every multiply, add, divide and square root
// on its own, on the host and in the set kernels alike (tests/test_collider_views_cpu.py restates it in numpy, byte for byte).
// Behind them the host steps of a set call from device memory (set_rows_device) and of its host variant (launch_row_chunks).
#pragma once
#include <initializer_list>

#include "body.h"

namespace tetsim {

// neither infinite nor NaN, by its bits
__host__ __device__ inline bool finite_value(double x) { return (__builtin_bit_cast(uint64_t, x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
__host__ __device__ inline bool finite_value(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

// ---- one collider -------------------------------------------------------------------------------------------------------------------------------
// why collider_view refuses, in the order it checks (a caller has its own text for each)
enum ColliderRefusal : int {
    kColliderOk = 0, kColliderKind, kColliderNonFinite, kColliderNegative, kColliderPlaneNormal, kColliderHalfExtent, kColliderZeroAxis, kColliderSkewedAxes
};

// v / sqrt(v . v) in f64; false for a zero vector
template <class T>
__host__ __device__ inline bool unit3(const T* v, double* out) {
    const double x = v[0], y = v[1], z = v[2];
    const double l2 = (x * x + y * y) + z * z;
    if (!(l2 > 0.0)) return false;
    const double l = sqrt(l2);
    out[0] = x / l; out[1] = y / l; out[2] = z / l;
    return true;
}

// A collider's fields (include/tetsim.h: TetSimCollider; kind as a value) -> the f64 view: checked as a whole -- every value finite, used by
// the kind or not -- plane normal and box axes normalised.  Returns kColliderOk and fills *o, or the first reason in ColliderRefusal's
// order; *o is then undefined.  T: double, the host's fields, or float, a row's -- every f32 is exactly a double, and a value is widened
// where it is read (a set kernel that widened its 21 floats in front of the call held them all in registers as doubles: 103 VGPRs for 78);
// the kind and finite checks decide the same either way, every other operation is f64.
template <class T>
__host__ __device__ inline int collider_view(T kind, const T* a, const T* b, const T* axes, T radius, T friction, const T* velocity, DevColliderD* o) {
    const bool known = kind == T(0) || kind == T(1) || kind == T(2) || kind == T(3);
    bool finite = true;   // (every field looked at before the first branch, in the fields' order in memory: a set kernel has its loads in flight together)
    for (int j = 0; j < 3; j++) finite = finite && finite_value(a[j]);
    for (int j = 0; j < 3; j++) finite = finite && finite_value(b[j]);
    for (int j = 0; j < 9; j++) finite = finite && finite_value(axes[j]);
    finite = finite && finite_value(radius) && finite_value(friction);
    for (int j = 0; j < 3; j++) finite = finite && finite_value(velocity[j]);
    if (!known) return kColliderKind;
    if (!finite) return kColliderNonFinite;
    const int32_t k = static_cast<int32_t>(kind);
    const bool box = k == TETSIM_COLLIDER_BOX, plane = k == TETSIM_COLLIDER_PLANE, round = !box && !plane;
    const double r = radius, fr = friction;
    if (fr < 0.0 || (round && r < 0.0)) return kColliderNegative;
    o->kind = k;
    o->pad = 0;
    o->radius = round ? r : 0.0;
    o->friction = fr;
    for (int j = 0; j < 3; j++) { o->a[j] = a[j]; o->b[j] = b[j]; o->v[j] = velocity[j]; }
    for (int j = 0; j < 9; j++) o->u[j] = 0.0;
    if (plane && !unit3(b, o->b)) return kColliderPlaneNormal;
    if (box) {
        for (int j = 0; j < 3; j++) {
            if (static_cast<double>(b[j]) < 0.0) return kColliderHalfExtent;
            if (!unit3(axes + 3 * j, o->u + 3 * j)) return kColliderZeroAxis;
        }
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; j < 3; j++) {
                const double* ui = o->u + 3 * i;
                const double* uj = o->u + 3 * j;
                if (fabs((ui[0] * uj[0] + ui[1] * uj[1]) + ui[2] * uj[2]) > 1e-5) return kColliderSkewedAxes;
            }
    }
    return kColliderOk;
}

// the f32 view: every value rounded once from the f64 view
__host__ __device__ inline DevColliderF collider_f32(const DevColliderD& o) {
    DevColliderF g;
    g.kind = o.kind;
    g.pad = 0;
    g.radius = static_cast<float>(o.radius);
    g.friction = static_cast<float>(o.friction);
    for (int j = 0; j < 3; j++) { g.a[j] = static_cast<float>(o.a[j]); g.b[j] = static_cast<float>(o.b[j]); g.v[j] = static_cast<float>(o.v[j]); }
    for (int j = 0; j < 9; j++) g.u[j] = static_cast<float>(o.u[j]);
    return g;
}

// ---- one row of parameters ------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kParamDoubles = TETSIM_BODY_PARAMS_WIDTH;
static_assert(kParamDoubles == 10u && sizeof(TetSimParams) == 8u * kParamDoubles && sizeof(BodyParamsD) == 8u * kParamDoubles, "a row is a TetSimParams");
static_assert(offsetof(TetSimParams, gravity) == 8u * TETSIM_BP_GRAVITY && offsetof(TetSimParams, friction) == 8u * TETSIM_BP_FRICTION &&
                  offsetof(TetSimParams, devCompliance) == 8u * TETSIM_BP_DEV_COMPLIANCE && offsetof(TetSimParams, volCompliance) == 8u * TETSIM_BP_VOL_COMPLIANCE &&
                  offsetof(TetSimParams, worldBounds) == 8u * TETSIM_BP_BOUNDS_LO && TETSIM_BP_BOUNDS_HI == TETSIM_BP_BOUNDS_LO + 3,
              "row layout");

// what the set calls refuse: a row with a non-finite value.  (The call's own TetSimParams are not checked: fill_params converts them as they are.)
__host__ __device__ inline bool params_finite(const double* r) {
    for (uint32_t j = 0; j < kParamDoubles; j++)
        if (!finite_value(r[j])) return false;
    return true;
}
// One row of ten doubles -> the two views: f64 the row as it stands, f32 every value rounded once from it.  fixed_bounds: the f32 view keeps
// the reference's constant box (dev_common.h: ref_fixed_lo / _hi), whatever the row says.
__host__ __device__ inline void params_views(const double* r, bool fixed_bounds, BodyParamsD* d, BodyParamsF* f) {
    d->gravity = r[TETSIM_BP_GRAVITY]; d->friction = r[TETSIM_BP_FRICTION];
    d->dev_compliance = r[TETSIM_BP_DEV_COMPLIANCE]; d->vol_compliance = r[TETSIM_BP_VOL_COMPLIANCE];
    f->gravity = static_cast<float>(d->gravity); f->friction = static_cast<float>(d->friction);
    f->dev_compliance = static_cast<float>(d->dev_compliance); f->vol_compliance = static_cast<float>(d->vol_compliance);
    for (int c = 0; c < 3; c++) {
        d->lo[c] = r[TETSIM_BP_BOUNDS_LO + c]; d->hi[c] = r[TETSIM_BP_BOUNDS_HI + c];
        f->lo[c] = fixed_bounds ? ref_fixed_lo(c) : static_cast<float>(d->lo[c]);
        f->hi[c] = fixed_bounds ? ref_fixed_hi(c) : static_cast<float>(d->hi[c]);
    }
    f->pad[0] = f->pad[1] = 0.0f;
}
// a POLAR_JACOBI handle created with TETSIM_FLAG_REF_FIXED_BOUNDS keeps the reference's constant box (SoftbodyGPU.js:347) in its f32 view
inline bool fixed_bounds(const tetsim_body* h) { return h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI && (h->opt.flags & TETSIM_FLAG_REF_FIXED_BOUNDS) != 0u; }

// ---- the host steps of a set call ---------------------------------------------------------------------------------------------------------------
// body_mask of a device-side call: null (every body), or `nb` bytes of device memory
inline int check_body_mask(tetsim_body* h, const void* mask, uint32_t nb) {
    if (!mask) return 0;
    return check_device_span(h, mask, nb, "body_mask", std::to_string(nb) + " bytes (one per body) do not fit the allocation it points into");
}
// the stride argument `name` of records of `row_bytes`: 0 (packed) or a multiple of `align` of at least the record
inline int check_record_stride(tetsim_body* h, const char* name, uint64_t stride, uint64_t row_bytes, uint32_t align) {
    if (record_stride_ok(stride, row_bytes, align)) return 0;
    return fail(h, TETSIM_EINVAL, std::string(name) + " must be 0 or a multiple of " + std::to_string(align) + " of at least " + std::to_string(row_bytes));
}
inline uint64_t resolved_stride(uint64_t stride, uint64_t row_bytes) { return stride ? stride : row_bytes; }

// a kernel with a lane per body, on h->stream
template <class Kernel, class... Args>
inline int launch_per_body(tetsim_body* h, uint32_t nb, Kernel kernel, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((nb + 255u) / 256u), dim3(256), 0, h->stream, args...);
    return launched(h);
}

// One array of a set call in the caller's device memory: `rows` records of `row_bytes`, `stride` apart as the caller passed it (0 = packed);
// stride_name: the argument's name in the refusal, null for an array that is always packed.
struct DeviceRows {
    const void* ptr;
    const char* name;
    uint64_t rows, row_bytes;
    uint32_t align;
    uint64_t stride;
    const char* stride_name;
};
// What a set call from device memory does behind its null checks, in the one order of refusals: the feature's state check, the strides, the
// handle's guard, every array's records, the mask; then -- every argument is good, only allocation and HIP itself can fail -- the table
// (ensure: the first call's may block), `launch` on h->stream under the caller's stream contract, and the feature's switch.
template <class State, class Ensure, class Launch>
inline int set_rows_device(tetsim_body* h, State&& check_state, std::initializer_list<DeviceRows> arrays, const void* body_mask, void* caller_stream, Ensure&& ensure,
                           Launch&& launch, bool* on) {
    if (int rc = check_state()) return rc;
    for (const DeviceRows& a : arrays)
        if (a.stride_name)
            if (int rc = check_record_stride(h, a.stride_name, a.stride, a.row_bytes, a.align)) return rc;
    if (int rc = device_call_guard(h)) return rc;
    for (const DeviceRows& a : arrays) {
        if (a.rows > 0xffffffffull) return fail(h, TETSIM_EINVAL, "too many rows");
        if (int rc = check_device_records(h, a.ptr, resolved_stride(a.stride, a.row_bytes), static_cast<uint32_t>(a.rows), a.row_bytes, a.align, a.name)) return rc;
    }
    if (int rc = check_body_mask(h, body_mask, num_bodies(h))) return rc;
    if (int rc = ensure()) return rc;
    const int rc = on_caller_stream(h, caller_stream, launch);
    if (rc == 0) *on = true;
    return rc;
}

// The host variant's rows travel as kernel arguments, a chunk of whole bodies per launch: kRows rows of kWidth values.
template <class T, uint32_t kWidth, uint32_t kRows>
struct RowChunk {
    T row[kRows][kWidth];
    static constexpr uint32_t rows = kRows, row_bytes = kWidth * sizeof(T);
};
// src: the host's packed rows, rows_per_body for each of nb bodies, or null (the chunks stay zero); launch(chunk, first body, bodies) on h->stream
template <class Chunk, class Launch>
inline int launch_row_chunks(tetsim_body* h, const void* src, uint32_t nb, uint32_t rows_per_body, Launch&& launch) {
    static_assert(sizeof(Chunk) + 64 <= kKernelArgLimit, "a chunk of rows is a kernel argument");
    const uint32_t per_launch = Chunk::rows / rows_per_body;
    for (uint32_t first = 0; first < nb; first += per_launch) {
        const uint32_t bodies = std::min(per_launch, nb - first);
        Chunk c{};
        if (src) std::memcpy(c.row, static_cast<const char*>(src) + static_cast<size_t>(first) * rows_per_body * Chunk::row_bytes, static_cast<size_t>(bodies) * rows_per_body * Chunk::row_bytes);
        launch(c, first, bodies);
    }
    return launched(h);
}

}  // namespace tetsim
