// touch.hip -- C ABI (include/tetsim.h, "touch sensing"): tetsim_touch_bodies_device / tetsim_read_body_touch / tetsim_touch_particles_device.
// A read-only query beside observe.hip: the signed distance and the outward normal of every particle against every collider its body's
// substeps walk -- the handle's list, or the body's compacted entries of the body-collider table while that is on, in the arithmetic view the
// handle holds (f32 or f64), widened to f64 -- reduced per body and slot (count, least distance, centroid, mean normal, mean relative
// velocity), or handed out per particle.  Positions and velocities as the export hands them out (export_sources, gathered through
// d_api2dev), ordered against the caller's stream as the export is.  f64 arithmetic, every operation rounded on its own (this unit is
// built with -ffp-contract=off); the fixed reduction tree over the particle chunks of body_reduce.h, no atomics: the same state gives the
// same bits, and a body of a batch the bits it gives alone.  No stepping kernel includes anything from here.
#include "body_reduce.h"
#include "collide.h"

using namespace tetsim;

namespace tetsim {
namespace {

constexpr uint32_t kSlotVals = 10;                                      // a slot's reduced doubles: [0] least sd, [1..3] S p, [4..6] S n, [7..9] S (v - V)
constexpr uint32_t kSlotCountAt = kSlotVals;                            // ... and behind them its touching particles (a 64-bit count in the double's place)
constexpr uint32_t kSlotPartial = kSlotVals + 1u;
// A chunk's partial row: [0] least sd of the chunk, [1] its touching particles (a count, likewise), then kSlotPartial doubles per slot; only
// the slots of the body's list are written and read.
constexpr uint32_t kHeadPartial = 2, kHeadCountAt = 1;
constexpr uint32_t kTouchPartial = kHeadPartial + kMaxColliders * kSlotPartial;
static_assert(TETSIM_TOUCH_SLOT_WIDTH == 12 && TETSIM_TOUCH_WIDTH == 4u + kMaxColliders * TETSIM_TOUCH_SLOT_WIDTH && TETSIM_TOUCH_PARTICLE_WIDTH == 8, "row layout");

// value 0 a minimum, the others sums (the head's single value is a minimum too)
struct TouchOps {
    static __device__ __forceinline__ double combine(double a, double b, uint32_t k) { return k == 0u ? fmin(a, b) : a + b; }
    static __device__ __forceinline__ double identity(uint32_t k) { return k == 0u ? INFINITY : 0.0; }
};

// The lists of a call, by value: the body-collider table while it is on (count != null), the handle's list otherwise -- Col is the view
// the handle holds.  A workgroup holds one body, so the index is uniform and the entries arrive by scalar loads.
template <class Col>
struct TouchLists {
    const uint32_t* count;     // [bodies], null: every body meets list[0 .. n)
    const Col* table;          // [bodies][kMaxColliders]
    uint32_t n, pad;
    Col list[kMaxColliders];
};
static_assert(sizeof(TouchLists<DevColliderD>) + 128 <= kKernelArgLimit, "the lists are a kernel argument");
template <class Col> __device__ __forceinline__ uint32_t list_count(const TouchLists<Col>& L, uint32_t body) { return L.count ? min(L.count[body], kMaxColliders) : L.n; }
template <class Col> __device__ __forceinline__ Col list_entry(const TouchLists<Col>& L, uint32_t body, uint32_t k) {
    if (L.count) return L.table[static_cast<size_t>(body) * kMaxColliders + k];
    return L.list[k];
}

// THE definition (tetsim.h restates it): signed distance and outward unit normal of the point (x, y, z) against one collider, in f64 on the
// collider's values widened to f64.  collide.h's hit test continued to the outside: where collide_f64 hits, sd < 0, -sd is its depth and
// n its normal.
template <class Col>
__device__ __forceinline__ void touch_sd(const double x, const double y, const double z, const Col& C, double& sd, double& nx, double& ny, double& nz) {
    using collide::js_max;
    using collide::js_min;
    const double a0 = C.a[0], a1 = C.a[1], a2 = C.a[2], b0 = C.b[0], b1 = C.b[1], b2 = C.b[2];
    if (C.kind == 0 || C.kind == 1) {
        double cx = a0, cy = a1, cz = a2;
        if (C.kind == 1) {
            const double abx = b0 - a0, aby = b1 - a1, abz = b2 - a2;
            const double ab2 = (abx * abx + aby * aby) + abz * abz;
            double t = 0.0;
            if (ab2 != 0.0) t = (((x - a0) * abx + (y - a1) * aby) + (z - a2) * abz) / ab2;
            t = js_min(js_max(t, 0.0), 1.0);
            cx = a0 + abx * t; cy = a1 + aby * t; cz = a2 + abz * t;
        }
        const double dx = x - cx, dy = y - cy, dz = z - cz;
        const double L = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
        sd = L - static_cast<double>(C.radius);
        const bool apart = L > 0.0;
        nx = apart ? dx / L : 0.0; ny = apart ? dy / L : 0.0; nz = apart ? dz / L : 0.0;
    } else if (C.kind == 2) {
        const double dx = x - a0, dy = y - a1, dz = z - a2;
        // (scalars, not arrays: the face is picked by selects, nothing is indexed by a run-time value)
        const double u00 = C.u[0], u01 = C.u[1], u02 = C.u[2], u10 = C.u[3], u11 = C.u[4], u12 = C.u[5], u20 = C.u[6], u21 = C.u[7], u22 = C.u[8];
        const double l0 = (dx * u00 + dy * u01) + dz * u02, l1 = (dx * u10 + dy * u11) + dz * u12, l2 = (dx * u20 + dy * u21) + dz * u22;
        const double g0 = b0 - __builtin_fabs(l0), g1 = b1 - __builtin_fabs(l1), g2 = b2 - __builtin_fabs(l2);
        if (g0 >= 0.0 && g1 >= 0.0 && g2 >= 0.0) {   // inside or on the box: the face the step would push through
            const bool one = g1 < g0;
            const double ga = one ? g1 : g0;
            const bool two = g2 < ga;
            const double gj = two ? g2 : ga;
            const double lj = two ? l2 : one ? l1 : l0;
            const double ux = two ? u20 : one ? u10 : u00, uy = two ? u21 : one ? u11 : u01, uz = two ? u22 : one ? u12 : u02;
            const bool plus = lj >= 0.0;
            sd = -gj;
            nx = plus ? ux : -ux; ny = plus ? uy : -uy; nz = plus ? uz : -uz;
        } else {                                     // outside: the distance to the nearest point of the box (a NaN g gives a NaN sd)
            const double o0 = js_max(-g0, 0.0), o1 = js_max(-g1, 0.0), o2 = js_max(-g2, 0.0);
            const double s0 = l0 >= 0.0 ? o0 : -o0, s1 = l1 >= 0.0 ? o1 : -o1, s2 = l2 >= 0.0 ? o2 : -o2;
            sd = __builtin_sqrt((o0 * o0 + o1 * o1) + o2 * o2);
            const double wx = ((0.0 + s0 * u00) + s1 * u10) + s2 * u20;
            const double wy = ((0.0 + s0 * u01) + s1 * u11) + s2 * u21;
            const double wz = ((0.0 + s0 * u02) + s1 * u12) + s2 * u22;
            nx = wx / sd; ny = wy / sd; nz = wz / sd;
        }
    } else {
        sd = ((x - a0) * b0 + (y - a1) * b1) + (z - a2) * b2;
        nx = b0; ny = b1; nz = b2;
    }
}

// First launch of the body rows: one workgroup per particle chunk, one lane per particle, slot by slot; the chunk's partial row leaves
// through thread 0.
template <class Col>
__global__ __launch_bounds__(256) void touch_chunks_kernel(const BodyChunk* __restrict__ chunks, const TouchLists<Col> L, const float4* __restrict__ pos,
                                                          const float4* __restrict__ vel, const uint32_t* __restrict__ map, const double margin,
                                                          double* __restrict__ partial) {
    __shared__ double lds[4][kSlotVals];
    __shared__ unsigned long long lds_n[4];
    const BodyChunk c = chunks[blockIdx.x];
    double* const row = partial + static_cast<uint64_t>(blockIdx.x) * kTouchPartial;
    const bool live = threadIdx.x < c.count;
    double x = 0.0, y = 0.0, z = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
    if (live) {
        const uint32_t r = c.first + threadIdx.x;
        const uint32_t i = map ? map[r] : r;
        const float4 p = pos[i], u = vel[i];
        x = p.x; y = p.y; z = p.z; ux = u.x; uy = u.y; uz = u.z;
    }
    const uint32_t slots = list_count(L, c.body);
    double nearest[1] = {INFINITY};
    uint32_t touching = 0u;
    for (uint32_t k = 0; k < slots; k++) {
        const Col C = list_entry(L, c.body, k);
        double v[kSlotVals];
#pragma unroll
        for (uint32_t j = 0; j < kSlotVals; j++) v[j] = TouchOps::identity(j);
        uint32_t n = 0u;
        if (live) {
            double sd, nx, ny, nz;
            touch_sd(x, y, z, C, sd, nx, ny, nz);
            v[0] = fmin(sd, INFINITY);   // (a NaN sd is no minimum)
            nearest[0] = fmin(nearest[0], sd);
            if (sd < margin) {
                n = 1u; touching = 1u;
                v[1] = x; v[2] = y; v[3] = z;
                v[4] = nx; v[5] = ny; v[6] = nz;
                v[7] = ux - static_cast<double>(C.v[0]); v[8] = uy - static_cast<double>(C.v[1]); v[9] = uz - static_cast<double>(C.v[2]);
            }
        }
        __syncthreads();   // (thread 0 has read the previous slot's LDS rows)
        block_reduce<TouchOps>(v, n, lds, lds_n);
        if (threadIdx.x == 0u) {
            double* const s = row + kHeadPartial + k * kSlotPartial;
#pragma unroll
            for (uint32_t j = 0; j < kSlotVals; j++) s[j] = v[j];
            s[kSlotCountAt] = __longlong_as_double(static_cast<long long>(n));
        }
    }
    __syncthreads();
    block_reduce<TouchOps>(nearest, touching, lds, lds_n);
    if (threadIdx.x == 0u) {
        row[0] = nearest[0];
        row[kHeadCountAt] = __longlong_as_double(static_cast<long long>(touching));
    }
}

// Second launch: one workgroup per body.  The fold of the body's partial rows (body_reduce.h: fold_rows), then the same tree, for the head
// and slot by slot; thread 0 divides and stores the finished row, every one of its TETSIM_TOUCH_WIDTH doubles.
template <class Col>
__global__ __launch_bounds__(256) void touch_finish_kernel(const BodyChunks* __restrict__ bodies, const TouchLists<Col> L, const double* __restrict__ partial,
                                                          char* __restrict__ dst, const uint64_t stride) {
    __shared__ double lds[4][kSlotVals];
    __shared__ unsigned long long lds_n[4];
    const BodyChunks b = bodies[blockIdx.x];
    double* const o = reinterpret_cast<double*>(dst + static_cast<uint64_t>(blockIdx.x) * stride);
    const uint32_t slots = list_count(L, blockIdx.x);
    double nearest[1];
    unsigned long long touching = 0ull;
    fold_rows<TouchOps, kTouchPartial>(b, partial, nearest, touching, kHeadCountAt);
    block_reduce<TouchOps>(nearest, touching, lds, lds_n);
    double least = INFINITY, least_slot = -1.0;
    for (uint32_t k = 0; k < slots; k++) {
        double v[kSlotVals];
        unsigned long long n = 0ull;
        fold_rows<TouchOps, kTouchPartial>(b, partial + kHeadPartial + k * kSlotPartial, v, n, kSlotCountAt);
        __syncthreads();
        block_reduce<TouchOps>(v, n, lds, lds_n);
        if (threadIdx.x != 0u) continue;
        double* const s = o + TETSIM_TOUCH_SLOT0 + k * TETSIM_TOUCH_SLOT_WIDTH;
        const double count = static_cast<double>(n);
        s[TETSIM_TOUCH_SLOT_KIND] = static_cast<double>(list_entry(L, blockIdx.x, k).kind);
        s[TETSIM_TOUCH_SLOT_COUNT] = count;
        s[TETSIM_TOUCH_SLOT_MIN_SD] = v[0];
#pragma unroll
        for (uint32_t j = 1; j < kSlotVals; j++) s[TETSIM_TOUCH_SLOT_CENTROID + (j - 1u)] = n ? v[j] / count : 0.0;
        if (v[0] < least) { least = v[0]; least_slot = static_cast<double>(k); }
    }
    if (threadIdx.x != 0u) return;
    for (uint32_t k = slots; k < kMaxColliders; k++) {
        double* const s = o + TETSIM_TOUCH_SLOT0 + k * TETSIM_TOUCH_SLOT_WIDTH;
        for (uint32_t j = 0; j < TETSIM_TOUCH_SLOT_WIDTH; j++) s[j] = 0.0;
        s[TETSIM_TOUCH_SLOT_KIND] = -1.0;
        s[TETSIM_TOUCH_SLOT_MIN_SD] = INFINITY;
    }
    o[TETSIM_TOUCH_TOUCHING] = static_cast<double>(touching);
    o[TETSIM_TOUCH_MIN_SD] = nearest[0];
    o[TETSIM_TOUCH_MIN_SLOT] = least_slot;
    o[TETSIM_TOUCH_SLOTS] = static_cast<double>(slots);
}

// The particle rows, one launch: one workgroup per particle chunk, one lane per particle, row r of dst = particle r of the caller's numbering.
template <class Col>
__global__ __launch_bounds__(256) void touch_particles_kernel(const BodyChunk* __restrict__ chunks, const TouchLists<Col> L, const float4* __restrict__ pos,
                                                             const uint32_t* __restrict__ map, const double margin, char* __restrict__ dst, const uint64_t stride) {
    const BodyChunk c = chunks[blockIdx.x];
    if (threadIdx.x >= c.count) return;
    const uint32_t r = c.first + threadIdx.x;
    const float4 p = pos[map ? map[r] : r];
    const double x = p.x, y = p.y, z = p.z;
    const uint32_t slots = list_count(L, c.body);
    double best = INFINITY, bx = 0.0, by = 0.0, bz = 0.0;
    int32_t slot = -1;
    uint32_t touched = 0u;
    for (uint32_t k = 0; k < slots; k++) {
        const Col C = list_entry(L, c.body, k);
        double sd, nx, ny, nz;
        touch_sd(x, y, z, C, sd, nx, ny, nz);
        if (sd < best) { best = sd; bx = nx; by = ny; bz = nz; slot = static_cast<int32_t>(k); }
        if (sd < margin) touched++;
    }
    float* const o = reinterpret_cast<float*>(dst + static_cast<uint64_t>(r) * stride);
    o[0] = static_cast<float>(best);
    o[1] = static_cast<float>(bx); o[2] = static_cast<float>(by); o[3] = static_cast<float>(bz);
    o[4] = static_cast<float>(slot);
    o[5] = static_cast<float>(touched);
    o[6] = 0.0f; o[7] = 0.0f;
}

// What the handle's first touch call builds and uploads (the only part of a call that blocks, with the export's events and index map): the
// particle chunk table (body_reduce.h) unless another call made it, and the scratch of the partial rows and the rows of the host read.
// All of it counts into TetSimInfo.device_bytes from then on.
int ensure_tables(tetsim_body* h) {
    TouchDev& d = h->touch;
    if (d.ready) return 0;
    if (int rc = ensure_chunk_table(h, kParticleChunks)) return rc;
    if (int rc = dev_alloc(h, &d.partial, static_cast<size_t>(h->chunk_table[kParticleChunks].n_chunks) * kTouchPartial)) return rc;
    if (int rc = dev_alloc(h, &d.rows, static_cast<size_t>(h->info.num_bodies) * TETSIM_TOUCH_WIDTH)) return rc;
    d.ready = true;   // (last: set only when every table is there)
    return 0;
}

// the lists the body's substeps read, in the view `Col`
inline const DevColliderF* host_list(const tetsim_body* h, const DevColliderF*) { return h->col; }
inline const DevColliderD* host_list(const tetsim_body* h, const DevColliderD*) { return h->d_col; }
inline const DevColliderF* body_table(const tetsim_body* h, const DevColliderF*) { return h->d_bcol_f; }
inline const DevColliderD* body_table(const tetsim_body* h, const DevColliderD*) { return h->d_bcol_d; }
template <class Col>
TouchLists<Col> lists_of(const tetsim_body* h) {
    TouchLists<Col> L{};
    if (h->body_colliders_on) {
        L.count = h->d_bcol_count;
        L.table = body_table(h, static_cast<const Col*>(nullptr));
    } else {
        L.n = std::min(h->n_colliders, kMaxColliders);
        for (uint32_t k = 0; k < L.n; k++) L.list[k] = host_list(h, static_cast<const Col*>(nullptr))[k];
    }
    return L;
}
inline bool f64_view(const tetsim_body* h) { return h->opt.solver == TETSIM_SOLVER_NEOHOOKEAN_GS && !h->fast; }

// the two launches of the body rows on h->stream: row b of dst = body b
template <class Col>
int enqueue_bodies(tetsim_body* h, double margin, void* dst, uint64_t stride) {
    const ChunkTable& vt = h->chunk_table[kParticleChunks];
    FieldSrc src[2];
    if (int rc = export_sources(h, {TETSIM_FIELD_POSITIONS, TETSIM_FIELD_VELOCITIES}, src)) return rc;
    const TouchLists<Col> L = lists_of<Col>(h);
    if (vt.n_chunks)
        hipLaunchKernelGGL(touch_chunks_kernel<Col>, dim3(vt.n_chunks), dim3(256), 0, h->stream, vt.chunks, L, src[0].src, src[1].src,
                           src[0].mapped ? h->d_api2dev : nullptr, margin, h->touch.partial);
    if (int rc = launched(h)) return rc;
    hipLaunchKernelGGL(touch_finish_kernel<Col>, dim3(h->info.num_bodies), dim3(256), 0, h->stream, vt.bodies, L, static_cast<const double*>(h->touch.partial),
                       static_cast<char*>(dst), stride);
    return launched(h);
}
int enqueue_bodies(tetsim_body* h, double margin, void* dst, uint64_t stride) {
    return f64_view(h) ? enqueue_bodies<DevColliderD>(h, margin, dst, stride) : enqueue_bodies<DevColliderF>(h, margin, dst, stride);
}

template <class Col>
int enqueue_particles(tetsim_body* h, double margin, void* dst, uint64_t stride) {
    const ChunkTable& vt = h->chunk_table[kParticleChunks];
    FieldSrc src[1];
    if (int rc = export_sources(h, {TETSIM_FIELD_POSITIONS}, src)) return rc;
    if (vt.n_chunks)
        hipLaunchKernelGGL(touch_particles_kernel<Col>, dim3(vt.n_chunks), dim3(256), 0, h->stream, vt.chunks, lists_of<Col>(h), src[0].src,
                           src[0].mapped ? h->d_api2dev : nullptr, margin, static_cast<char*>(dst), stride);
    return launched(h);
}

int check_margin(tetsim_body* h, double margin) {
    if (!std::isfinite(margin)) return fail(h, TETSIM_EINVAL, "margin must be finite");
    return 0;
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_touch_bodies_device(tetsim_handle h, double margin, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (int rc = check_margin(h, margin)) return rc;
    uint64_t stride;
    if (int rc = check_dst_rows(h, dst, row_stride, h->info.num_bodies, 8ull * TETSIM_TOUCH_WIDTH, 8u, &stride)) return rc;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_tables(h)) return rc;
    return on_caller_stream(h, caller_stream, [&] { return enqueue_bodies(h, margin, dst, stride); });
}

int tetsim_read_body_touch(tetsim_handle h, double margin, double* out) {
    if (!h) return TETSIM_EINVAL;
    if (!out) return fail(h, TETSIM_EINVAL, "out is null");
    if (int rc = check_margin(h, margin)) return rc;
    if (int rc = device_call_guard(h)) return rc;
    if (int rc = ensure_tables(h)) return rc;
    return read_back(h, out, h->touch.rows, static_cast<size_t>(h->info.num_bodies) * TETSIM_TOUCH_WIDTH,
                     [&] { return enqueue_bodies(h, margin, h->touch.rows, 8ull * TETSIM_TOUCH_WIDTH); });
}

int tetsim_touch_particles_device(tetsim_handle h, double margin, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (int rc = check_margin(h, margin)) return rc;
    uint64_t stride;
    if (int rc = check_dst_rows(h, dst, row_stride, h->info.owned_particles, 4ull * TETSIM_TOUCH_PARTICLE_WIDTH, 4u, &stride)) return rc;
    // ---- every argument is good
    if (int rc = ensure_tables(h)) return rc;
    return on_caller_stream(h, caller_stream, [&] {
        return f64_view(h) ? enqueue_particles<DevColliderD>(h, margin, dst, stride) : enqueue_particles<DevColliderF>(h, margin, dst, stride);
    });
}

}  // extern "C"
