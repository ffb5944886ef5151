// body_params.hip -- physics parameters per body of a batch (tetsim_set_body_params / _device): gravity, friction, the two compliances and
// the world bounds.  The table the substep kernels read in place of the call's TetSimParams (dev_common.h: body_params_row,
// body_params_polar; pj_quad.hip: load_qparams; nh_kernels.inc: load_vparams_of, body_compliances) is made here: a row per body in the
// view the handle's arithmetic reads -- f64 is the caller's row as it stands, f32 every value rounded once from it, the casts fill_params
// makes -- indexed through the particle -> body array the body grabs use too (body_grabs.hip: ensure_particle_bodies) and, in the
// Neo-Hookean tet solves, through a tet -> body array in the device's tet order.  One set kernel, a lane per body; bp_row below is the
// routine that checks and rounds a row, compiled for both sides: the host variant checks its rows with it, the kernel converts with it.
#include "body.h"

using namespace tetsim;

namespace tetsim {
namespace {

constexpr uint32_t kRowDoubles = TETSIM_BODY_PARAMS_WIDTH, kRowBytes = 8u * kRowDoubles;
static_assert(kRowDoubles == 10u && sizeof(TetSimParams) == kRowBytes && sizeof(BodyParamsD) == kRowBytes, "a row is a TetSimParams");
static_assert(offsetof(TetSimParams, gravity) == 8u * TETSIM_BP_GRAVITY && offsetof(TetSimParams, friction) == 8u * TETSIM_BP_FRICTION &&
                  offsetof(TetSimParams, devCompliance) == 8u * TETSIM_BP_DEV_COMPLIANCE && offsetof(TetSimParams, volCompliance) == 8u * TETSIM_BP_VOL_COMPLIANCE &&
                  offsetof(TetSimParams, worldBounds) == 8u * TETSIM_BP_BOUNDS_LO && TETSIM_BP_BOUNDS_HI == TETSIM_BP_BOUNDS_LO + 3,
              "row layout");

__host__ __device__ inline bool row_finite(double x) { return (__builtin_bit_cast(uint64_t, x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// One row of ten doubles -> the two views.  false for a row with a non-finite value (the views are then undefined).  fixed_bounds: a
// POLAR_JACOBI handle created with TETSIM_FLAG_REF_FIXED_BOUNDS keeps the reference's constant box (SoftbodyGPU.js:347) in its f32
// view, whatever the row says -- fill_params' rule.
__host__ __device__ inline bool bp_row(const double* r, bool fixed_bounds, BodyParamsD* d, BodyParamsF* f) {
    for (uint32_t j = 0; j < kRowDoubles; j++)
        if (!row_finite(r[j])) return false;
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
    return true;
}

// row r of body b into the view the handle keeps (the other pointer is null); a row with a non-finite value leaves the body's row in place
__device__ inline void bp_set_body(const double* r, bool fixed_bounds, uint32_t b, BodyParamsF* __restrict__ f, BodyParamsD* __restrict__ d) {
    BodyParamsD od;
    BodyParamsF of;
    if (!bp_row(r, fixed_bounds, &od, &of)) return;
    if (d) d[b] = od;
    if (f) f[b] = of;
}

// One lane per body, rows in the caller's device memory; a body the mask leaves out keeps its row.
__global__ __launch_bounds__(256) void bp_rows_kernel(const char* __restrict__ rows, uint64_t stride, const uint8_t* __restrict__ mask, uint32_t fixed_bounds,
                                                      BodyParamsF* __restrict__ f, BodyParamsD* __restrict__ d, uint32_t bodies) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= bodies) return;
    if (mask && mask[b] == 0) return;
    const double* const src = reinterpret_cast<const double*>(rows + static_cast<uint64_t>(b) * stride);
    double r[kRowDoubles];
    for (uint32_t j = 0; j < kRowDoubles; j++) r[j] = src[j];
    bp_set_body(r, fixed_bounds != 0u, b, f, d);
}
// The host variant's rows travel as kernel arguments, a chunk per launch (checked on the host with the same routine)
constexpr uint32_t kChunkRows = 40;
struct RowChunk { double row[kChunkRows][kRowDoubles]; };
static_assert(sizeof(RowChunk) + 64 <= kKernelArgLimit, "a chunk of rows is a kernel argument");
__global__ __launch_bounds__(64) void bp_rows_value_kernel(RowChunk c, uint32_t first, uint32_t bodies, uint32_t fixed_bounds, BodyParamsF* __restrict__ f, BodyParamsD* __restrict__ d) {
    const uint32_t i = threadIdx.x;
    if (i >= bodies || i >= kChunkRows) return;
    bp_set_body(c.row[i], fixed_bounds != 0u, first + i, f, d);
}
// the first set call's defaults: one row for every body
__global__ __launch_bounds__(256) void bp_fill_kernel(TetSimParams p, uint32_t fixed_bounds, BodyParamsF* __restrict__ f, BodyParamsD* __restrict__ d, uint32_t bodies) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= bodies) return;
    bp_set_body(reinterpret_cast<const double*>(&p), fixed_bounds != 0u, b, f, d);
}
// the body of every tet in the device's tet order (Neo-Hookean: solve order), from the first corner's body: a constant
__global__ __launch_bounds__(256) void bp_tet_body_kernel(const int4* __restrict__ tet_idx, const uint32_t* __restrict__ particle_body, uint32_t* __restrict__ tet_body, uint32_t nt) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e < nt) tet_body[e] = particle_body[static_cast<uint32_t>(tet_idx[e].x)];
}

bool fixed_bounds(const tetsim_body* h) { return h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI && (h->opt.flags & TETSIM_FLAG_REF_FIXED_BOUNDS) != 0u; }

// the table, every body at tetsim_default_params() (the first set call: allocates, and the particle -> body array may upload, so it may
// block).  Filled on the handle's stream, in front of the set kernel.
int ensure_table(tetsim_body* h) {
    if (h->d_bp_f || h->d_bp_d) return 0;
    if (int rc = ensure_particle_bodies(h)) return rc;
    const uint32_t nb = num_bodies(h);
    const bool neohookean = h->opt.solver == TETSIM_SOLVER_NEOHOOKEAN_GS;
    const bool f64_view = neohookean && !h->fast;
    BodyParamsF* df = nullptr;
    BodyParamsD* dd = nullptr;
    uint32_t* dt = nullptr;
    if (f64_view) { if (int rc = dev_alloc(h, &dd, nb)) return rc; }
    else if (int rc = dev_alloc(h, &df, nb)) return rc;
    if (neohookean && h->nh.nt != 0u) {
        if (int rc = dev_alloc(h, &dt, h->nh.nt)) return rc;
        hipLaunchKernelGGL(bp_tet_body_kernel, dim3((h->nh.nt + 255u) / 256u), dim3(256), 0, h->stream, h->nh.tet_idx, h->d_grab_body, dt, h->nh.nt);
    }
    TetSimParams p;
    tetsim_default_params(&p);
    hipLaunchKernelGGL(bp_fill_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, h->stream, p, fixed_bounds(h) ? 1u : 0u, df, dd, nb);
    if (int rc = launched(h)) return rc;
    h->d_tet_body = dt;
    h->d_bp_d = dd;
    h->d_bp_f = df;   // (set last: the table exists)
    return 0;
}

int check_state(tetsim_body* h) {
    if (h->partitioned || !h->group.empty()) return fail(h, TETSIM_ESTATE, "body parameters on a partitioned body are not supported (the call's params serve every partition)");
    return 0;
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_set_body_params(tetsim_handle h, const double* rows) {
    if (!h) return TETSIM_EINVAL;
    HIPCHK(h, hipSetDevice(h->opt.device));
    if (!rows) {   // OFF: host state; the table keeps its rows
        h->body_params_on = false;
        return 0;
    }
    if (int rc = check_state(h)) return rc;
    const uint32_t nb = num_bodies(h);
    for (uint32_t b = 0; b < nb; b++) {
        BodyParamsD d;
        BodyParamsF f;
        if (!bp_row(rows + static_cast<size_t>(b) * kRowDoubles, false, &d, &f)) return fail(h, TETSIM_EINVAL, "body " + std::to_string(b) + ": non-finite value in its row of parameters");
    }
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_table(h)) return rc;
    const uint32_t fixed = fixed_bounds(h) ? 1u : 0u;
    for (uint32_t first = 0; first < nb; first += kChunkRows) {
        const uint32_t bodies = std::min(kChunkRows, nb - first);
        RowChunk c{};
        std::memcpy(c.row, rows + static_cast<size_t>(first) * kRowDoubles, static_cast<size_t>(bodies) * kRowBytes);
        hipLaunchKernelGGL(bp_rows_value_kernel, dim3(1), dim3(64), 0, h->stream, c, first, bodies, fixed, h->d_bp_f, h->d_bp_d);
    }
    if (int rc = launched(h)) return rc;
    h->body_params_on = true;
    return 0;
}

int tetsim_set_body_params_device(tetsim_handle h, const void* rows, uint64_t row_stride, const void* body_mask, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!rows) {
        if (int rc = device_call_guard(h)) return rc;
        return tetsim_set_body_params(h, nullptr);
    }
    if (int rc = check_state(h)) return rc;
    if (!record_stride_ok(row_stride, kRowBytes, 8u)) return fail(h, TETSIM_EINVAL, "row_stride must be 0 or a multiple of 8 of at least 80");
    if (int rc = device_call_guard(h)) return rc;
    const uint32_t nb = num_bodies(h);
    const uint64_t stride = row_stride ? row_stride : kRowBytes;
    if (int rc = check_device_records(h, rows, stride, nb, kRowBytes, 8u, "rows")) return rc;
    if (body_mask) {
        if (int rc = check_device_span(h, body_mask, nb, "body_mask", std::to_string(nb) + " bytes (one per body) do not fit the allocation it points into")) return rc;
    }
    // ---- every argument is good
    if (int rc = ensure_table(h)) return rc;
    const int rc = on_caller_stream(h, caller_stream, [&]() -> int {
        hipLaunchKernelGGL(bp_rows_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, h->stream, static_cast<const char*>(rows), stride, static_cast<const uint8_t*>(body_mask),
                           fixed_bounds(h) ? 1u : 0u, h->d_bp_f, h->d_bp_d, nb);
        return launched(h);
    });
    if (rc == 0) h->body_params_on = true;
    return rc;
}

}  // extern "C"
