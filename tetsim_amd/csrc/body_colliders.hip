// body_colliders.hip -- up to eight kinematic colliders per body of a batch (tetsim_set_body_colliders / _device).  The table the particle
// passes read in place of the handle's list (dev_common.h: body_colliders_pick; collide.h: collide_particle_*; pj_quad.hip:
// pjq_vertex_update; nh_kernels.inc: post_vertex) is made here: per body a count and kMaxColliders compacted entries, in the view the
// handle's arithmetic reads, indexed through the particle -> body array the body grabs use too (body_grabs.hip: ensure_particle_bodies).
// One set kernel, a lane per body, does per row what tetsim_set_colliders does per collider on the host, with the routine it uses:
// body_rows.h: collider_view, compiled for both sides.  bcol_row below hands it a row's 21 floats, which it widens to double as it reads
// them; the host variant checks its rows with it, the kernel converts with it.  Built with -ffp-contract=off, as tetsim_visual.hip is: the two views equal the ones
// tetsim_set_colliders makes of the same numbers, bit for bit.
#include "body_rows.h"

using namespace tetsim;

namespace tetsim {

const char* const kBodyCollidersOn = "body colliders are on (tetsim_set_body_colliders): one kind of list at a time -- switch them off first (count 0 stays legal)";

namespace {

constexpr uint32_t kRowFloats = TETSIM_BODY_COLLIDER_FLOATS, kRowBytes = 4u * kRowFloats;
static_assert(kRowFloats == 24u && kMaxColliders == TETSIM_MAX_COLLIDERS, "row layout");

// One row of 24 floats -> the f64 view of its collider.  Returns 1 and fills *o; 0 for an empty slot (kind -1, nothing else is looked at);
// minus collider_view's reason for a row tetsim_set_colliders would refuse (kRowRefusal[-code - 1] says why), *o is then undefined.
__host__ __device__ inline int bcol_row(const float* r, DevColliderD* o) {
    if (r[0] == -1.0f) return 0;
    const int why = collider_view(r[0], r + 1, r + 4, r + 7, r[16], r[17], r + 18, o);
    return why == kColliderOk ? 1 : -why;
}
const char* const kRowRefusal[] = {"unknown kind (0, 1, 2, 3, or -1 for an empty slot)", "non-finite value", "negative radius or friction", "zero-length plane normal",
                                   "negative half-extent", "zero-length box axis", "box axes are not orthogonal"};

// The rows of ONE body -> its list: the rows the host would accept, compacted, in slot order; a refused row is an empty slot.
// row(k): the address of the body's row k.  f / d: the view the handle keeps (the other one is null).
template <class Row>
__device__ inline void bcol_set_body(const Row& row, uint32_t per_body, uint32_t b, uint32_t* __restrict__ count, DevColliderF* __restrict__ f, DevColliderD* __restrict__ d) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < per_body && k < kMaxColliders; k++) {
        const float* src = row(k);
        float r[kRowFloats];
        for (uint32_t j = 0; j < 21u; j++) r[j] = src[j];   // (floats 21..23 are never read)
        DevColliderD o;
        if (bcol_row(r, &o) != 1) continue;
        const size_t at = static_cast<size_t>(b) * kMaxColliders + n;
        if (d) d[at] = o;
        if (f) f[at] = collider_f32(o);
        n++;
    }
    count[b] = n;
}

// One lane per body, rows in the caller's device memory; a body the mask leaves out keeps its whole list.
__global__ __launch_bounds__(256) void bcol_rows_kernel(const char* __restrict__ rows, uint64_t stride, uint32_t per_body, const uint8_t* __restrict__ mask,
                                                        uint32_t* __restrict__ count, DevColliderF* __restrict__ f, DevColliderD* __restrict__ d, uint32_t bodies) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= bodies) return;
    if (mask && mask[b] == 0) return;
    const char* const mine = rows + static_cast<uint64_t>(b) * per_body * stride;
    bcol_set_body([&](uint32_t k) { return reinterpret_cast<const float*>(mine + static_cast<uint64_t>(k) * stride); }, per_body, b, count, f, d);
}
// The host variant's rows travel as kernel arguments, a chunk of whole bodies per launch (checked on the host with the same routine)
constexpr uint32_t kChunkRows = 40;   // 40 x 96 bytes: five bodies of eight rows
using Chunk = RowChunk<float, kRowFloats, kChunkRows>;
static_assert(kChunkRows >= kMaxColliders, "a chunk holds a whole body");
__global__ __launch_bounds__(64) void bcol_rows_value_kernel(Chunk c, uint32_t per_body, uint32_t first, uint32_t bodies, uint32_t* __restrict__ count,
                                                             DevColliderF* __restrict__ f, DevColliderD* __restrict__ d) {
    const uint32_t i = threadIdx.x;
    if (i >= bodies || (i + 1u) * per_body > kChunkRows) return;
    bcol_set_body([&](uint32_t k) { return static_cast<const float*>(c.row[i * per_body + k]); }, per_body, first + i, count, f, d);
}
// OFF: every body empty
__global__ __launch_bounds__(256) void bcol_clear_kernel(uint32_t* __restrict__ count, uint32_t bodies) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < bodies) count[b] = 0u;
}

// the table, every body empty (the first set call: allocates, and the particle -> body array may upload, so it may block).  Only the counts
// need a value: entries behind a body's count are never read.  They are cleared on the handle's stream, in front of the set kernel.
int ensure_table(tetsim_body* h) {
    if (h->d_bcol_count) return 0;
    if (int rc = ensure_particle_bodies(h)) return rc;
    const uint32_t nb = num_bodies(h);
    const bool f64_view = h->opt.solver == TETSIM_SOLVER_NEOHOOKEAN_GS && !h->fast;
    DevColliderF* df = nullptr;
    DevColliderD* dd = nullptr;
    uint32_t* dc = nullptr;
    if (f64_view) { if (int rc = dev_alloc(h, &dd, static_cast<size_t>(nb) * kMaxColliders)) return rc; }
    else if (int rc = dev_alloc(h, &df, static_cast<size_t>(nb) * kMaxColliders)) return rc;
    if (int rc = dev_alloc(h, &dc, nb)) return rc;
    if (int rc = launch_per_body(h, nb, bcol_clear_kernel, dc, nb)) return rc;
    h->d_bcol_f = df;
    h->d_bcol_d = dd;
    h->d_bcol_count = dc;   // (set last: the table exists)
    return 0;
}

// what either set call refuses whatever its rows are
int check_state(tetsim_body* h, uint32_t per_body) {
    if (h->partitioned || !h->group.empty()) return fail(h, TETSIM_ESTATE, "body colliders on a partitioned body are not supported (tetsim_set_colliders on each partition)");
    if (h->n_colliders != 0u) return fail(h, TETSIM_ESTATE, "the handle's collider list is set (tetsim_set_colliders): one kind of list at a time -- clear it first (count 0)");
    if (per_body == 0u || per_body > kMaxColliders) return fail(h, TETSIM_EINVAL, "per_body must be 1 .. TETSIM_MAX_COLLIDERS");
    return 0;
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_set_body_colliders(tetsim_handle h, const float* rows, uint32_t per_body) {
    if (!h) return TETSIM_EINVAL;
    HIPCHK(h, hipSetDevice(h->opt.device));
    const uint32_t nb = num_bodies(h);
    if (!rows) {   // OFF: host state; every body's list goes back to empty (a table that was never made holds nothing)
        h->body_colliders_on = false;
        return h->d_bcol_count ? launch_per_body(h, nb, bcol_clear_kernel, h->d_bcol_count, nb) : 0;
    }
    if (int rc = check_state(h, per_body)) return rc;
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t k = 0; k < per_body; k++) {
            DevColliderD o;
            const int code = bcol_row(rows + (static_cast<size_t>(b) * per_body + k) * kRowFloats, &o);
            if (code < 0) return fail(h, TETSIM_EINVAL, "body " + std::to_string(b) + ", slot " + std::to_string(k) + ": " + kRowRefusal[-code - 1]);
        }
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_table(h)) return rc;
    if (int rc = launch_row_chunks<Chunk>(h, rows, nb, per_body, [&](const Chunk& c, uint32_t first, uint32_t bodies) {
            hipLaunchKernelGGL(bcol_rows_value_kernel, dim3(1), dim3(64), 0, h->stream, c, per_body, first, bodies, h->d_bcol_count, h->d_bcol_f, h->d_bcol_d);
        })) return rc;
    h->body_colliders_on = true;
    return 0;
}

int tetsim_set_body_colliders_device(tetsim_handle h, const void* rows, uint64_t row_stride, uint32_t per_body, const void* body_mask, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!rows) {
        if (int rc = device_call_guard(h)) return rc;
        return tetsim_set_body_colliders(h, nullptr, 0u);
    }
    const uint32_t nb = num_bodies(h);
    return set_rows_device(
        h, [&] { return check_state(h, per_body); }, {{rows, "rows", static_cast<uint64_t>(nb) * per_body, kRowBytes, 4u, row_stride, "row_stride"}}, body_mask, caller_stream,
        [&] { return ensure_table(h); },
        [&] {
            return launch_per_body(h, nb, bcol_rows_kernel, static_cast<const char*>(rows), resolved_stride(row_stride, kRowBytes), per_body, static_cast<const uint8_t*>(body_mask),
                                   h->d_bcol_count, h->d_bcol_f, h->d_bcol_d, nb);
        },
        &h->body_colliders_on);
}

}  // extern "C"
