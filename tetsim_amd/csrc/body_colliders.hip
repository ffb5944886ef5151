// body_colliders.hip -- up to eight kinematic colliders per body of a batch (tetsim_set_body_colliders / _device).  The table the particle
// passes read in place of the handle's list (dev_common.h: body_colliders_pick; collide.h: collide_particle_*; pj_quad.hip:
// pjq_vertex_update; nh_kernels.inc: post_vertex) is made here: per body a count and kMaxColliders compacted entries, in the view the
// handle's arithmetic reads, indexed through the particle -> body array the body grabs use too (body_grabs.hip: ensure_particle_bodies).
// One set kernel, a lane per body, does per row what tetsim_set_colliders does per collider on the host -- bcol_row below IS that
// routine, compiled for both sides: the host variant checks its rows with it, the kernel converts with it.  Built with
// -ffp-contract=off: the f64 normalisation rounds every multiply, add, divide and square root on its own, so the two views equal the
// ones tetsim_set_colliders makes of the same numbers, bit for bit.
#include "body.h"

using namespace tetsim;

namespace tetsim {

const char* const kBodyCollidersOn = "body colliders are on (tetsim_set_body_colliders): one kind of list at a time -- switch them off first (count 0 stays legal)";

namespace {

constexpr uint32_t kRowFloats = TETSIM_BODY_COLLIDER_FLOATS, kRowBytes = 4u * kRowFloats;
static_assert(kRowFloats == 24u && kMaxColliders == TETSIM_MAX_COLLIDERS, "row layout");

__host__ __device__ inline bool row_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

// v / sqrt(v . v) in f64; false for a zero vector (tetsim_set_colliders: unit)
__host__ __device__ inline bool row_unit(const double* v, double* out) {
    const double l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (!(l2 > 0.0)) return false;
    const double l = sqrt(l2);
    for (int j = 0; j < 3; j++) out[j] = v[j] / l;
    return true;
}

// One row of 24 floats -> the f64 view of its collider.  Returns 1 and fills *o; 0 for an empty slot (kind -1, nothing else is looked at);
// a negative number for a row tetsim_set_colliders would refuse (kRowRefusal[-code - 1] says why), *o is then undefined.
__host__ __device__ inline int bcol_row(const float* r, DevColliderD* o) {
    const float kf = r[0];
    if (kf == -1.0f) return 0;
    if (!(kf == 0.0f || kf == 1.0f || kf == 2.0f || kf == 3.0f)) return -1;
    for (uint32_t j = 1; j < 21u; j++)
        if (!row_finite(r[j])) return -2;
    const int32_t kind = static_cast<int32_t>(kf);
    const bool box = kind == TETSIM_COLLIDER_BOX, plane = kind == TETSIM_COLLIDER_PLANE, round = !box && !plane;
    const double radius = r[16], friction = r[17];
    if (friction < 0.0 || (round && radius < 0.0)) return -3;
    double a[3], b[3], u[9], v[3];
    for (int j = 0; j < 3; j++) { a[j] = r[1 + j]; b[j] = r[4 + j]; v[j] = r[18 + j]; }
    for (int j = 0; j < 9; j++) u[j] = r[7 + j];
    o->kind = kind;
    o->pad = 0;
    o->radius = round ? radius : 0.0;
    o->friction = friction;
    for (int j = 0; j < 3; j++) { o->a[j] = a[j]; o->b[j] = b[j]; o->v[j] = v[j]; }
    for (int j = 0; j < 9; j++) o->u[j] = 0.0;
    if (plane && !row_unit(b, o->b)) return -4;
    if (box) {
        for (int j = 0; j < 3; j++) {
            if (b[j] < 0.0) return -5;
            if (!row_unit(u + 3 * j, o->u + 3 * j)) return -6;
        }
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; j < 3; j++) {
                const double* ui = o->u + 3 * i;
                const double* uj = o->u + 3 * j;
                if (fabs((ui[0] * uj[0] + ui[1] * uj[1]) + ui[2] * uj[2]) > 1e-5) return -7;
            }
    }
    return 1;
}
const char* const kRowRefusal[] = {"unknown kind (0, 1, 2, 3, or -1 for an empty slot)", "non-finite value", "negative radius or friction", "zero-length plane normal",
                                   "negative half-extent", "zero-length box axis", "box axes are not orthogonal"};

// the f32 view: every value rounded once from the f64 view
__device__ inline DevColliderF bcol_f32(const DevColliderD& o) {
    DevColliderF g;
    g.kind = o.kind;
    g.pad = 0;
    g.radius = static_cast<float>(o.radius);
    g.friction = static_cast<float>(o.friction);
    for (int j = 0; j < 3; j++) { g.a[j] = static_cast<float>(o.a[j]); g.b[j] = static_cast<float>(o.b[j]); g.v[j] = static_cast<float>(o.v[j]); }
    for (int j = 0; j < 9; j++) g.u[j] = static_cast<float>(o.u[j]);
    return g;
}

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
        if (f) f[at] = bcol_f32(o);
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
struct RowChunk { float row[kChunkRows][kRowFloats]; };
static_assert(sizeof(RowChunk) + 64 <= kKernelArgLimit && kChunkRows >= kMaxColliders, "a chunk of rows is a kernel argument");
__global__ __launch_bounds__(64) void bcol_rows_value_kernel(RowChunk c, uint32_t per_body, uint32_t first, uint32_t bodies, uint32_t* __restrict__ count,
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
    hipLaunchKernelGGL(bcol_clear_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, h->stream, dc, nb);
    if (int rc = launched(h)) return rc;
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
        if (!h->d_bcol_count) return 0;
        hipLaunchKernelGGL(bcol_clear_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, h->stream, h->d_bcol_count, nb);
        return launched(h);
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
    const uint32_t per_launch = kChunkRows / per_body;
    for (uint32_t first = 0; first < nb; first += per_launch) {
        const uint32_t bodies = std::min(per_launch, nb - first);
        RowChunk c{};
        std::memcpy(c.row, rows + static_cast<size_t>(first) * per_body * kRowFloats, static_cast<size_t>(bodies) * per_body * kRowBytes);
        hipLaunchKernelGGL(bcol_rows_value_kernel, dim3(1), dim3(64), 0, h->stream, c, per_body, first, bodies, h->d_bcol_count, h->d_bcol_f, h->d_bcol_d);
    }
    if (int rc = launched(h)) return rc;
    h->body_colliders_on = true;
    return 0;
}

int tetsim_set_body_colliders_device(tetsim_handle h, const void* rows, uint64_t row_stride, uint32_t per_body, const void* body_mask, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!rows) {
        if (int rc = device_call_guard(h)) return rc;
        return tetsim_set_body_colliders(h, nullptr, 0u);
    }
    if (int rc = check_state(h, per_body)) return rc;
    if (!record_stride_ok(row_stride, kRowBytes, 4u)) return fail(h, TETSIM_EINVAL, "row_stride must be 0 or a multiple of 4 of at least 96");
    if (int rc = device_call_guard(h)) return rc;
    const uint32_t nb = num_bodies(h);
    const uint64_t stride = row_stride ? row_stride : kRowBytes;
    if (static_cast<uint64_t>(nb) * per_body > 0xffffffffull) return fail(h, TETSIM_EINVAL, "too many rows");
    if (int rc = check_device_records(h, rows, stride, nb * per_body, kRowBytes, 4u, "rows")) return rc;
    if (body_mask) {
        if (int rc = check_device_span(h, body_mask, nb, "body_mask", std::to_string(nb) + " bytes (one per body) do not fit the allocation it points into")) return rc;
    }
    // ---- every argument is good
    if (int rc = ensure_table(h)) return rc;
    const int rc = on_caller_stream(h, caller_stream, [&]() -> int {
        hipLaunchKernelGGL(bcol_rows_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, h->stream, static_cast<const char*>(rows), stride, per_body,
                           static_cast<const uint8_t*>(body_mask), h->d_bcol_count, h->d_bcol_f, h->d_bcol_d, nb);
        return launched(h);
    });
    if (rc == 0) h->body_colliders_on = true;
    return rc;
}

}  // extern "C"
