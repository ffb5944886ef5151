// observe.hip -- C ABI, part 7 (include/tetsim.h): tetsim_observe_bodies_device / tetsim_read_body_observations.  One row of
// TETSIM_OBS_WIDTH doubles per body of the handle -- mass, mass centre and its velocity, volume, rest volume, the worst tet's volume ratio,
// the inverted tets, the box of the particles, the fastest particle, the non-finite particles -- computed on the device from the rows the
// export hands out (device_io.hip: resolve_field / prepare_fields, gathered through d_api2dev), so no stepping path's tet order matters, and
// ordered against the caller's stream as the export is (on_caller_stream).  f64 arithmetic on the stored f32 values, every operation
// rounded on its own (this unit is built with -ffp-contract=off); the fixed reduction tree over the chunks of body_reduce.h, no atomics: the
// same state gives the same bits, and a body of a batch the bits it gives alone.  See body.h.
#include "body_reduce.h"

using namespace tetsim;

namespace tetsim {
namespace {

constexpr uint32_t kObsPartial = 12;    // doubles of a chunk's partial row (below)
constexpr uint32_t kObsTetVals = 10, kObsVertVals = 7;
// A tet chunk's partial row: [0] sum 4w, [1..3] sum w * (x0+x1+x2+x3), [4..6] the same of the velocities, [7] sum V, [8] sum V0,
// [9] min V/V0, [10] inverted tets (a 64-bit count in the double's place).  A particle chunk's: [0..2] box min, [3..5] box max,
// [6] max speed^2, [7] non-finite particles (a count, likewise).  The tet chunks' rows come first, then the particle chunks'.
constexpr uint32_t kTetCountAt = 10, kVertCountAt = 7;

__device__ __forceinline__ double obs_dot(double ux, double uy, double uz, double vx, double vy, double vz) { return (ux * vx + uy * vy) + uz * vz; }
// dot(b - a, cross(c - a, d - a)) / 6 of four float4 corners
__device__ __forceinline__ double obs_volume(const float4& a, const float4& b, const float4& c, const float4& d) {
    const double e1x = static_cast<double>(b.x) - a.x, e1y = static_cast<double>(b.y) - a.y, e1z = static_cast<double>(b.z) - a.z;
    const double e2x = static_cast<double>(c.x) - a.x, e2y = static_cast<double>(c.y) - a.y, e2z = static_cast<double>(c.z) - a.z;
    const double e3x = static_cast<double>(d.x) - a.x, e3y = static_cast<double>(d.y) - a.y, e3z = static_cast<double>(d.z) - a.z;
    const double cx = e2y * e3z - e2z * e3y, cy = e2z * e3x - e2x * e3z, cz = e2x * e3y - e2y * e3x;
    return obs_dot(e1x, e1y, e1z, cx, cy, cz) / 6.0;
}
__device__ __forceinline__ double obs_corner_sum(float a, float b, float c, float d) {
    return ((static_cast<double>(a) + b) + c) + d;
}

// which of the partial row's values are sums, minima, maxima
struct TetOps {
    static __device__ __forceinline__ double combine(double a, double b, uint32_t k) { return k == 9u ? fmin(a, b) : a + b; }
    static __device__ __forceinline__ double identity(uint32_t k) { return k == 9u ? INFINITY : 0.0; }
};
struct VertOps {
    static __device__ __forceinline__ double combine(double a, double b, uint32_t k) { return k < 3u ? fmin(a, b) : fmax(a, b); }
    static __device__ __forceinline__ double identity(uint32_t k) { return k < 3u ? INFINITY : k < 6u ? -INFINITY : 0.0; }
};

// First launch: one workgroup per chunk -- the tet chunks, then the particle chunks -- one lane per tet / particle; the chunk's partial row
// leaves through thread 0.
__global__ __launch_bounds__(256) void observe_chunks_kernel(const BodyChunk* __restrict__ tet_chunks, uint32_t n_tet_chunks, const BodyChunk* __restrict__ vert_chunks,
                                                            const int4* __restrict__ tets, const double* __restrict__ v0, const float4* __restrict__ pos,
                                                            const float4* __restrict__ vel, const uint32_t* __restrict__ map, double density, double* __restrict__ partial) {
    __shared__ double lds[4][kObsTetVals];
    __shared__ unsigned long long lds_n[4];
    const bool of_tets = blockIdx.x < n_tet_chunks;   // (uniform)
    const BodyChunk c = of_tets ? tet_chunks[blockIdx.x] : vert_chunks[blockIdx.x - n_tet_chunks];
    double* const row = partial + static_cast<uint64_t>(blockIdx.x) * kObsPartial;
    const bool live = threadIdx.x < c.count;
    const uint32_t r = c.first + threadIdx.x;
    if (of_tets) {
        double v[kObsTetVals];
#pragma unroll
        for (uint32_t k = 0; k < kObsTetVals; k++) v[k] = TetOps::identity(k);
        uint32_t inverted = 0u;
        if (live) {
            const int4 id = tets[r];
            const double V0 = v0[r];
            const uint32_t i0 = map ? map[id.x] : id.x, i1 = map ? map[id.y] : id.y, i2 = map ? map[id.z] : id.z, i3 = map ? map[id.w] : id.w;
            const float4 x0 = pos[i0], x1 = pos[i1], x2 = pos[i2], x3 = pos[i3];
            const float4 u0 = vel[i0], u1 = vel[i1], u2 = vel[i2], u3 = vel[i3];
            const double w = (density * V0) / 4.0;
            const double V = obs_volume(x0, x1, x2, x3);
            v[0] = 4.0 * w;
            v[1] = w * obs_corner_sum(x0.x, x1.x, x2.x, x3.x);
            v[2] = w * obs_corner_sum(x0.y, x1.y, x2.y, x3.y);
            v[3] = w * obs_corner_sum(x0.z, x1.z, x2.z, x3.z);
            v[4] = w * obs_corner_sum(u0.x, u1.x, u2.x, u3.x);
            v[5] = w * obs_corner_sum(u0.y, u1.y, u2.y, u3.y);
            v[6] = w * obs_corner_sum(u0.z, u1.z, u2.z, u3.z);
            v[7] = V;
            v[8] = V0;
            if (V0 != 0.0) {
                const double ratio = V / V0;
                v[9] = fmin(ratio, INFINITY);   // (a NaN ratio is left out of the minimum, as fmin leaves it out further up the tree)
                inverted = ratio <= 0.0 ? 1u : 0u;
            }
        }
        __syncthreads();   // (the kernel's barriers are what they were when the tree began with one)
        block_reduce<TetOps>(v, inverted, lds, lds_n);
        if (threadIdx.x == 0u) {
#pragma unroll
            for (uint32_t k = 0; k < kObsTetVals; k++) row[k] = v[k];
            row[kTetCountAt] = __longlong_as_double(static_cast<long long>(inverted));
            row[11] = 0.0;
        }
    } else {
        double v[kObsVertVals];
#pragma unroll
        for (uint32_t k = 0; k < kObsVertVals; k++) v[k] = VertOps::identity(k);
        uint32_t nonfinite = 0u;
        if (live) {
            const uint32_t i = map ? map[r] : r;
            const float4 x = pos[i], u = vel[i];
            if (isfinite(x.x) && isfinite(x.y) && isfinite(x.z) && isfinite(u.x) && isfinite(u.y) && isfinite(u.z)) {
                const double ux = u.x, uy = u.y, uz = u.z;
                v[0] = v[3] = x.x; v[1] = v[4] = x.y; v[2] = v[5] = x.z;
                v[6] = (ux * ux + uy * uy) + uz * uz;
            } else nonfinite = 1u;
        }
        __syncthreads();
        block_reduce<VertOps>(v, nonfinite, lds, lds_n);
        if (threadIdx.x == 0u) {
#pragma unroll
            for (uint32_t k = 0; k < kObsVertVals; k++) row[k] = v[k];
            row[kVertCountAt] = __longlong_as_double(static_cast<long long>(nonfinite));
#pragma unroll
            for (uint32_t k = kVertCountAt + 1u; k < kObsPartial; k++) row[k] = 0.0;
        }
    }
}

// Second launch: one workgroup per body.  The fold of the body's partial rows (body_reduce.h: fold_rows), then the same tree, for its tets
// and for its particles; thread 0 divides and stores the finished row.
__global__ __launch_bounds__(256) void observe_finish_kernel(const BodyChunks* __restrict__ tet_bodies, const BodyChunks* __restrict__ vert_bodies, const double* __restrict__ tet_partial,
                                                            const double* __restrict__ vert_partial, char* __restrict__ dst, uint64_t stride) {
    __shared__ double lds[4][kObsTetVals];
    __shared__ unsigned long long lds_n[4];
    double t[kObsTetVals], p[kObsVertVals];
    unsigned long long inverted = 0ull, nonfinite = 0ull;
    fold_rows<TetOps, kObsPartial>(tet_bodies[blockIdx.x], tet_partial, t, inverted, kTetCountAt);
    fold_rows<VertOps, kObsPartial>(vert_bodies[blockIdx.x], vert_partial, p, nonfinite, kVertCountAt);
    block_reduce<TetOps>(t, inverted, lds, lds_n);
    __syncthreads();   // (thread 0 has read the tets' LDS rows before the particles' are written)
    block_reduce<VertOps>(p, nonfinite, lds, lds_n);
    if (threadIdx.x != 0u) return;
    double* const o = reinterpret_cast<double*>(dst + static_cast<uint64_t>(blockIdx.x) * stride);
    const double mass = t[0];
    const bool massless = mass == 0.0;
    o[TETSIM_OBS_MASS] = mass;
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) {
        o[TETSIM_OBS_COM + k] = massless ? 0.0 : t[1u + k] / mass;
        o[TETSIM_OBS_VCOM + k] = massless ? 0.0 : t[4u + k] / mass;
        o[TETSIM_OBS_AABB_MIN + k] = p[k];
        o[TETSIM_OBS_AABB_MAX + k] = p[3u + k];
    }
    o[TETSIM_OBS_VOLUME] = t[7];
    o[TETSIM_OBS_REST_VOLUME] = t[8];
    o[TETSIM_OBS_MIN_VOLUME_RATIO] = t[9];
    o[TETSIM_OBS_INVERTED_TETS] = static_cast<double>(inverted);
    o[TETSIM_OBS_MAX_SPEED2] = p[6];
    o[TETSIM_OBS_NONFINITE] = static_cast<double>(nonfinite);
    o[TETSIM_OBS_RESERVED] = 0.0;
}

// What the handle's first observation builds and uploads (the only part of a call that blocks, with the export's events and index map):
// both chunk tables (body_reduce.h) unless another call made them, per tet its four API particle ids and V0, and the scratch of the
// partial rows and the rows of the host read.  All of it counts into TetSimInfo.device_bytes from then on.
int ensure_tables(tetsim_body* h) {
    ObsDev& d = h->obs;
    if (d.ready) return 0;
    if (int rc = ensure_chunk_table(h, kTetChunks)) return rc;
    if (int rc = ensure_chunk_table(h, kParticleChunks)) return rc;
    const uint32_t nt = h->info.num_elems;
    std::vector<int4> ids(nt);
    std::vector<double> v0(nt);
    for (uint32_t e = 0; e < nt; e++) {
        const int32_t* t = &h->h_tets[4ull * e];
        ids[e] = make_int4(t[0], t[1], t[2], t[3]);
        v0[e] = rest_volume(h->h_verts.data(), t);   // (body.h)
    }
    const size_t n_chunks = static_cast<size_t>(h->chunk_table[kTetChunks].n_chunks) + h->chunk_table[kParticleChunks].n_chunks;
    int4* d_ids = nullptr; double* d_v0 = nullptr;
    if (int rc = dev_alloc(h, &d_ids, ids.size())) return rc;
    if (int rc = dev_alloc(h, &d_v0, v0.size())) return rc;
    if (int rc = dev_alloc(h, &d.partial, n_chunks * kObsPartial)) return rc;
    if (int rc = dev_alloc(h, &d.rows, static_cast<size_t>(h->info.num_bodies) * TETSIM_OBS_WIDTH)) return rc;
    if (int rc = upload(h, d_ids, ids)) return rc;
    if (int rc = upload(h, d_v0, v0)) return rc;
    d.tets = d_ids; d.v0 = d_v0;
    d.ready = true;   // (last: set only when every table is there)
    return 0;
}

// the two launches on h->stream: row b of dst = body b
int enqueue_observation(tetsim_body* h, void* dst, uint64_t stride) {
    const ObsDev& d = h->obs;
    const ChunkTable &tt = h->chunk_table[kTetChunks], &vt = h->chunk_table[kParticleChunks];
    FieldSrc src[2];
    if (int rc = export_sources(h, {TETSIM_FIELD_POSITIONS, TETSIM_FIELD_VELOCITIES}, src)) return rc;
    if (tt.n_chunks + vt.n_chunks)
        hipLaunchKernelGGL(observe_chunks_kernel, dim3(tt.n_chunks + vt.n_chunks), dim3(256), 0, h->stream, tt.chunks, tt.n_chunks, vt.chunks, static_cast<const int4*>(d.tets),
                           d.v0, src[0].src, src[1].src, src[0].mapped ? h->d_api2dev : nullptr, h->opt.density, d.partial);
    if (int rc = launched(h)) return rc;
    hipLaunchKernelGGL(observe_finish_kernel, dim3(h->info.num_bodies), dim3(256), 0, h->stream, tt.bodies, vt.bodies, static_cast<const double*>(d.partial),
                       static_cast<const double*>(d.partial) + static_cast<size_t>(tt.n_chunks) * kObsPartial, static_cast<char*>(dst), stride);
    return launched(h);
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_observe_bodies_device(tetsim_handle h, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    uint64_t stride;
    if (int rc = check_dst_rows(h, dst, row_stride, h->info.num_bodies, 8ull * TETSIM_OBS_WIDTH, 8u, &stride)) return rc;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_tables(h)) return rc;
    return on_caller_stream(h, caller_stream, [&] { return enqueue_observation(h, dst, stride); });
}

int tetsim_read_body_observations(tetsim_handle h, double* out) {
    if (!h) return TETSIM_EINVAL;
    if (!out) return fail(h, TETSIM_EINVAL, "out is null");
    if (int rc = device_call_guard(h)) return rc;
    if (int rc = ensure_tables(h)) return rc;
    return read_back(h, out, h->obs.rows, static_cast<size_t>(h->info.num_bodies) * TETSIM_OBS_WIDTH, [&] { return enqueue_observation(h, h->obs.rows, 8ull * TETSIM_OBS_WIDTH); });
}

}  // extern "C"
