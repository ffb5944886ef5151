// body_params.hip -- physics parameters per body of a batch (tetsim_set_body_params / _device): gravity, friction, the two compliances and
// the world bounds.  The table the substep kernels read in place of the call's TetSimParams (dev_common.h: body_params_row,
// body_params_polar; pj_quad.hip: load_qparams; nh_kernels.inc: load_vparams_of, body_compliances) is made here: a row per body in the
// view the handle's arithmetic reads -- f64 is the caller's row as it stands, f32 every value rounded once from it -- indexed through the
// particle -> body array the body grabs use too (body_grabs.hip: ensure_particle_bodies) and, in the Neo-Hookean tet solves, through a
// tet -> body array in the device's tet order.  One set kernel, a lane per body.  The routines are body_rows.h's, compiled for both sides:
// params_finite is what a set call refuses (the host variant checks its rows with it, the kernel skips a row with it), params_views
// the conversion -- the one fill_params (tetsim_api.hip) makes of the call's TetSimParams, fixed-bounds rule included.
#include "body_rows.h"

using namespace tetsim;

namespace tetsim {
namespace {

constexpr uint32_t kRowDoubles = kParamDoubles, kRowBytes = 8u * kRowDoubles;

// row r of body b into the view the handle keeps (the other pointer is null); a row with a non-finite value leaves the body's row in place
__device__ inline void bp_set_body(const double* r, bool fixed_bounds, uint32_t b, BodyParamsF* __restrict__ f, BodyParamsD* __restrict__ d) {
    BodyParamsD od;
    BodyParamsF of;
    if (!params_finite(r)) return;
    params_views(r, fixed_bounds, &od, &of);
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
using Chunk = RowChunk<double, kRowDoubles, kChunkRows>;
__global__ __launch_bounds__(64) void bp_rows_value_kernel(Chunk c, uint32_t first, uint32_t bodies, uint32_t fixed_bounds, BodyParamsF* __restrict__ f, BodyParamsD* __restrict__ d) {
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
    if (int rc = launch_per_body(h, nb, bp_fill_kernel, p, fixed_bounds(h) ? 1u : 0u, df, dd, nb)) return rc;
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
    for (uint32_t b = 0; b < nb; b++)
        if (!params_finite(rows + static_cast<size_t>(b) * kRowDoubles)) return fail(h, TETSIM_EINVAL, "body " + std::to_string(b) + ": non-finite value in its row of parameters");
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_table(h)) return rc;
    const uint32_t fixed = fixed_bounds(h) ? 1u : 0u;
    if (int rc = launch_row_chunks<Chunk>(h, rows, nb, 1u, [&](const Chunk& c, uint32_t first, uint32_t bodies) {
            hipLaunchKernelGGL(bp_rows_value_kernel, dim3(1), dim3(64), 0, h->stream, c, first, bodies, fixed, h->d_bp_f, h->d_bp_d);
        })) return rc;
    h->body_params_on = true;
    return 0;
}

int tetsim_set_body_params_device(tetsim_handle h, const void* rows, uint64_t row_stride, const void* body_mask, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!rows) {
        if (int rc = device_call_guard(h)) return rc;
        return tetsim_set_body_params(h, nullptr);
    }
    const uint32_t nb = num_bodies(h);
    return set_rows_device(
        h, [&] { return check_state(h); }, {{rows, "rows", nb, kRowBytes, 8u, row_stride, "row_stride"}}, body_mask, caller_stream, [&] { return ensure_table(h); },
        [&] {
            return launch_per_body(h, nb, bp_rows_kernel, static_cast<const char*>(rows), resolved_stride(row_stride, kRowBytes), static_cast<const uint8_t*>(body_mask),
                                   fixed_bounds(h) ? 1u : 0u, h->d_bp_f, h->d_bp_d, nb);
        },
        &h->body_params_on);
}

}  // extern "C"
