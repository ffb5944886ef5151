// body_grabs.hip -- one held particle per body of a batch (tetsim_set_body_grabs / _device) and the nearest particle of every body on the
// device (tetsim_nearest_particles_device).  The table the particle passes read (dev_common.h: grab_pick; nh_kernels.inc: post_vertex;
// pj_quad.hip: load_qparams) is made here: the body of every particle in DEVICE particle order, a constant, and one 16-byte row per body,
// {device particle or -1, target xyz}, written by one small kernel per set call.  Built with -ffp-contract=off: the nearest query's squared
// distance is tetsim_nearest_particle's (util_kernels.hip: nearest_kernel), every multiply and add rounded on its own.  The host steps of
// the set calls are body_rows.h's (set_rows_device, launch_row_chunks), shared with the other per-body tables.  See body.h.
#include "body_reduce.h"
#include "body_rows.h"

#include <cfloat>

using namespace tetsim;

namespace tetsim {

const char* const kBodyGrabsOn = "body grabs are on (tetsim_set_body_grabs): one kind of grab at a time -- switch them off first";

uint32_t num_bodies(const tetsim_body* h) { return is_batch(h) ? static_cast<uint32_t>(h->batch_first_vert.size() - 1u) : 1u; }

// [bodies + 1] first particle of every body (caller's numbering) on the device, and the index map: what both features start from
int ensure_body_first(tetsim_body* h) {
    if (h->d_body_first) return ensure_index_map(h);
    std::vector<uint32_t> first_vert, first_tet;
    body_ranges(h, &first_vert, &first_tet);
    if (int rc = dev_alloc(h, &h->d_body_first, first_vert.size())) return rc;
    if (int rc = upload(h, h->d_body_first, first_vert)) return rc;
    return ensure_index_map(h);
}

// the body of every particle in DEVICE particle order, a constant: what the particle passes index the per-body tables with (body grabs,
// body colliders -- whichever is set first makes it; its address never changes)
int ensure_particle_bodies(tetsim_body* h) {
    if (h->d_grab_body) return 0;
    if (int rc = ensure_body_first(h)) return rc;
    std::vector<uint32_t> first_vert, first_tet;
    body_ranges(h, &first_vert, &first_tet);
    const uint32_t nv = h->info.num_particles, nb = num_bodies(h);
    std::vector<uint32_t> body(nv);
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t a = first_vert[b]; a < first_vert[b + 1u]; a++) body[h->api2dev.empty() ? a : h->api2dev[a]] = b;
    uint32_t* d_body = nullptr;
    if (int rc = dev_alloc(h, &d_body, body.size())) return rc;
    if (int rc = upload(h, d_body, body)) return rc;
    h->d_grab_body = d_body;
    return 0;
}

namespace {

constexpr uint32_t kNearChunk = kBodyChunk;   // particles per candidate, counted from the body's own first particle: nearest_kernel's blocks of the body alone

// One lane per body: the caller's row -> the table's.  first[b]: the body's first particle in the caller's numbering; map: caller's
// particle -> device particle (null = identity).  A row the table cannot hold -- an index outside the body, a non-finite target --
// becomes "none"; a body the mask leaves out keeps its row.
__global__ __launch_bounds__(256) void grab_rows_kernel(const int32_t* __restrict__ particles, const char* __restrict__ targets, uint64_t stride,
                                                        const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first,
                                                        const uint32_t* __restrict__ map, int4* __restrict__ rows, uint32_t bodies) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= bodies) return;
    if (mask && mask[b] == 0) return;
    const int32_t p = particles[b];
    const float* const t = reinterpret_cast<const float*>(targets + static_cast<uint64_t>(b) * stride);
    const float x = t[0], y = t[1], z = t[2];
    const uint32_t f0 = first[b], n = first[b + 1u] - f0;
    const bool ok = p >= 0 && static_cast<uint32_t>(p) < n && finite_f32(x) && finite_f32(y) && finite_f32(z);
    int4 row = make_int4(-1, 0, 0, 0);
    if (ok) {
        const uint32_t a = f0 + static_cast<uint32_t>(p);
        row = make_int4(static_cast<int32_t>(map ? map[a] : a), __float_as_int(x), __float_as_int(y), __float_as_int(z));
    }
    rows[b] = row;
}
// The host variant's rows travel as kernel arguments, a chunk per launch (checked and translated on the host); `none`: every row to "none"
constexpr uint32_t kRowsPerLaunch = 128;
using Chunk = RowChunk<int4, 1u, kRowsPerLaunch>;
__global__ __launch_bounds__(kRowsPerLaunch) void grab_rows_value_kernel(Chunk c, int4* __restrict__ rows, uint32_t first, uint32_t count, uint32_t none) {
    const uint32_t i = threadIdx.x;
    if (i < count) rows[first + i] = none ? make_int4(-1, 0, 0, 0) : c.row[i][0];
}

// ---- nearest particle per body: argmin of Softbody.js:279-291 over each body's particles -------------------------------------------------
// One workgroup per chunk of 256 particles of ONE body: nearest_kernel's candidate -- f64, a0*a0 + a1*a1 + a2*a2, NaN never picked, the lowest
// index among equals -- for the chunk, against the body's own point.  chunks: the particle chunk table (body_reduce.h).
__global__ __launch_bounds__(kNearChunk) void near_chunk_kernel(const float4* __restrict__ pos, const uint32_t* __restrict__ map, const BodyChunk* __restrict__ chunks,
                                                                const char* __restrict__ points, uint64_t stride, double* __restrict__ best_d2, uint32_t* __restrict__ best_id) {
    __shared__ double s_d[kNearChunk];
    __shared__ uint32_t s_i[kNearChunk];
    const BodyChunk ck = chunks[blockIdx.x];
    const uint32_t a = ck.first + threadIdx.x;
    const float* const q = reinterpret_cast<const float*>(points + static_cast<uint64_t>(ck.body) * stride);
    const double px = static_cast<double>(q[0]), py = static_cast<double>(q[1]), pz = static_cast<double>(q[2]);
    double d2 = DBL_MAX;
    if (threadIdx.x < ck.count) {
        const float4 p = pos[map ? map[a] : a];
        const double a0 = px - static_cast<double>(p.x), a1 = py - static_cast<double>(p.y), a2 = pz - static_cast<double>(p.z);
        d2 = a0 * a0 + a1 * a1 + a2 * a2;
        if (d2 != d2) d2 = DBL_MAX;   // `d2 < minD2` is false for NaN: such a particle is never picked
    }
    s_d[threadIdx.x] = d2;
    s_i[threadIdx.x] = a;
    __syncthreads();
    for (uint32_t w = kNearChunk / 2u; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double o = s_d[threadIdx.x + w];
            const uint32_t oi = s_i[threadIdx.x + w];
            if (o < s_d[threadIdx.x] || (o == s_d[threadIdx.x] && oi < s_i[threadIdx.x])) { s_d[threadIdx.x] = o; s_i[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { best_d2[blockIdx.x] = s_d[0]; best_id[blockIdx.x] = s_i[0]; }
}
// One lane per body: its chunks' candidates in index order, `<` keeps the first minimum -- the loop the host runs behind nearest_kernel
__global__ __launch_bounds__(256) void near_body_kernel(const double* __restrict__ best_d2, const uint32_t* __restrict__ best_id, const BodyChunks* __restrict__ body_chunks,
                                                        const uint32_t* __restrict__ first, int32_t* __restrict__ ids, double* __restrict__ dist2, uint32_t bodies) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= bodies) return;
    const BodyChunks mine = body_chunks[b];
    double best = DBL_MAX;
    int32_t id = -1;
    for (uint32_t c = mine.chunk0; c < mine.chunk0 + mine.chunks; c++) {
        const double d = best_d2[c];
        if (d < best) { best = d; id = static_cast<int32_t>(best_id[c] - first[b]); }
    }
    ids[b] = id;
    if (dist2) dist2[b] = best;
}

// the table, every row "none" (the first set call: allocates and uploads, so it may block)
int ensure_grab_table(tetsim_body* h) {
    if (h->d_grab_rows) return 0;
    if (int rc = ensure_particle_bodies(h)) return rc;
    const std::vector<int4> none(num_bodies(h), make_int4(-1, 0, 0, 0));
    int4* d_rows = nullptr;
    if (int rc = dev_alloc(h, &d_rows, none.size())) return rc;
    if (int rc = upload(h, d_rows, none)) return rc;
    h->d_grab_rows = d_rows;
    return 0;
}

// what either set call refuses whatever its rows are
int check_grab_state(tetsim_body* h) {
    if (h->partitioned || !h->group.empty()) return fail(h, TETSIM_ESTATE, "body grabs on a partitioned body are not supported (tetsim_set_grab on each partition)");
    if (h->opt.flags & TETSIM_FLAG_REF_GRAB_TEXEL) return fail(h, TETSIM_ESTATE, "body grabs on a TETSIM_FLAG_REF_GRAB_TEXEL handle are not supported (its quirk picks other particles, in host arithmetic)");
    if (h->grab_global >= 0) return fail(h, TETSIM_ESTATE, "a handle grab is set (tetsim_set_grab): one kind of grab at a time -- release it first (id -1)");
    if (h->body_pins_on) return fail(h, TETSIM_ESTATE, kBodyPinsOn);
    return 0;
}

// rows [first, first + count) from the host, or "none" for all of them, on h->stream
int launch_value_rows(tetsim_body* h, const std::vector<int4>* rows, uint32_t nb) {
    return launch_row_chunks<Chunk>(h, rows ? rows->data() : nullptr, nb, 1u, [&](const Chunk& c, uint32_t first, uint32_t count) {
        hipLaunchKernelGGL(grab_rows_value_kernel, dim3(1), dim3(kRowsPerLaunch), 0, h->stream, c, h->d_grab_rows, first, count, rows ? 0u : 1u);
    });
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_set_body_grabs(tetsim_handle h, const int32_t* particles, const float* targets) {
    if (!h) return TETSIM_EINVAL;
    HIPCHK(h, hipSetDevice(h->opt.device));
    const uint32_t nb = num_bodies(h);
    if (!particles) {   // OFF: host state; the rows go back to "none" (a table that was never made holds nothing)
        h->body_grabs_on = false;
        return h->d_grab_rows ? launch_value_rows(h, nullptr, nb) : 0;
    }
    if (!targets) return fail(h, TETSIM_EINVAL, "targets is null");
    if (int rc = check_grab_state(h)) return rc;
    std::vector<uint32_t> first_vert, first_tet;
    body_ranges(h, &first_vert, &first_tet);
    std::vector<int4> rows(nb, make_int4(-1, 0, 0, 0));
    for (uint32_t b = 0; b < nb; b++) {
        const int32_t p = particles[b];
        const float* t = targets + 3ull * b;
        const std::string at = "body " + std::to_string(b) + ": ";
        if (p == -1) continue;
        if (p < 0 || static_cast<uint32_t>(p) >= first_vert[b + 1u] - first_vert[b]) return fail(h, TETSIM_EINVAL, at + "particle index outside the body (-1 = not held)");
        if (!std::isfinite(t[0]) || !std::isfinite(t[1]) || !std::isfinite(t[2])) return fail(h, TETSIM_EINVAL, at + "non-finite target");
        const uint32_t a = first_vert[b] + static_cast<uint32_t>(p);
        int4 r;
        r.x = static_cast<int32_t>(h->api2dev.empty() ? a : h->api2dev[a]);
        std::memcpy(&r.y, t, 3 * sizeof(float));
        rows[b] = r;
    }
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_grab_table(h)) return rc;
    if (int rc = launch_value_rows(h, &rows, nb)) return rc;
    h->body_grabs_on = true;
    return 0;
}

int tetsim_set_body_grabs_device(tetsim_handle h, const void* particles, const void* targets, uint64_t target_stride, const void* body_mask, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!particles) {
        if (int rc = device_call_guard(h)) return rc;
        return tetsim_set_body_grabs(h, nullptr, nullptr);
    }
    if (!targets) return fail(h, TETSIM_EINVAL, "targets is null");
    const uint32_t nb = num_bodies(h);
    return set_rows_device(
        h, [&] { return check_grab_state(h); }, {{particles, "particles", nb, 4u, 4u, 0u, nullptr}, {targets, "targets", nb, 12u, 4u, target_stride, "target_stride"}}, body_mask,
        caller_stream, [&] { return ensure_grab_table(h); },
        [&] {
            return launch_per_body(h, nb, grab_rows_kernel, static_cast<const int32_t*>(particles), static_cast<const char*>(targets), resolved_stride(target_stride, 12u),
                                   static_cast<const uint8_t*>(body_mask), h->d_body_first, h->d_api2dev, h->d_grab_rows, nb);
        },
        &h->body_grabs_on);
}

int tetsim_nearest_particles_device(tetsim_handle h, const void* points, uint64_t point_stride, void* ids, void* dist2, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!points || !ids) return fail(h, TETSIM_EINVAL, "null argument");
    if (int rc = check_record_stride(h, "point_stride", point_stride, 12u, 4u)) return rc;
    if (int rc = device_call_guard(h)) return rc;
    const uint32_t nb = num_bodies(h);
    const uint64_t stride = resolved_stride(point_stride, 12u);
    if (int rc = check_device_records(h, points, stride, nb, 12u, 4u, "points")) return rc;
    if (int rc = check_device_records(h, ids, 4u, nb, 4u, 4u, "ids")) return rc;
    if (dist2) { if (int rc = check_device_records(h, dist2, 8u, nb, 8u, 8u, "dist2")) return rc; }
    // ---- every argument is good
    if (int rc = ensure_body_first(h)) return rc;
    if (int rc = ensure_chunk_table(h, kParticleChunks)) return rc;
    const ChunkTable& t = h->chunk_table[kParticleChunks];
    if (!h->d_near_id) {   // (the first call: a candidate per chunk; the id's pointer is set last)
        if (int rc = dev_alloc(h, &h->d_near_d2, t.n_chunks)) return rc;
        if (int rc = dev_alloc(h, &h->d_near_id, t.n_chunks)) return rc;
    }
    return on_caller_stream(h, caller_stream, [&]() -> int {
        if (t.n_chunks)
            hipLaunchKernelGGL(near_chunk_kernel, dim3(t.n_chunks), dim3(kNearChunk), 0, h->stream, current_positions(h), h->d_api2dev, t.chunks,
                               static_cast<const char*>(points), stride, h->d_near_d2, h->d_near_id);
        hipLaunchKernelGGL(near_body_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, h->stream, h->d_near_d2, h->d_near_id, t.bodies, h->d_body_first,
                           static_cast<int32_t*>(ids), static_cast<double*>(dist2), nb);
        return launched(h);
    });
}

}  // extern "C"
