// observe.hip -- C ABI, part 7 (include/tetsim.h): tetsim_observe_bodies_device / tetsim_read_body_observations.  One row of
// TETSIM_OBS_WIDTH doubles per body of the handle -- mass, mass centre and its velocity, volume, rest volume, the worst tet's volume ratio,
// the inverted tets, the box of the particles, the fastest particle, the non-finite particles -- computed on the device from the rows the
// export hands out (device_io.hip: resolve_field / prepare_fields, gathered through d_api2dev), so no stepping path's tet order matters, and
// ordered against the caller's stream as the export is (on_caller_stream).  f64 arithmetic on the stored f32 values, every operation
// rounded on its own (this unit is built with -ffp-contract=off); a fixed reduction tree, no atomics: the same state gives the same bits,
// and a body of a batch the bits it gives alone.  See body.h.
#include "body.h"

using namespace tetsim;

namespace tetsim {
namespace {

constexpr uint32_t kObsChunk = 256;     // tets / particles of one workgroup; a body's chunks count from ITS first tet / particle
constexpr uint32_t kObsPartial = 12;    // doubles of a chunk's partial row (below)
constexpr uint32_t kObsTetVals = 10, kObsVertVals = 7;
enum : uint32_t { kObsTets = 0u, kObsVerts = 1u };
// A tet chunk's partial row: [0] sum 4w, [1..3] sum w * (x0+x1+x2+x3), [4..6] the same of the velocities, [7] sum V, [8] sum V0,
// [9] min V/V0, [10] inverted tets (a 64-bit count in the double's place).  A particle chunk's: [0..2] box min, [3..5] box max,
// [6] max speed^2, [7] non-finite particles (a count, likewise).
constexpr uint32_t kTetCountAt = 10, kVertCountAt = 7;

struct ObsChunk { uint32_t body, first, count, kind; };          // first: the chunk's first tet / particle in the API's numbering
struct ObsBody { uint32_t tet_chunk0, tet_chunks, vert_chunk0, vert_chunks; };   // the body's partial rows

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
__device__ __forceinline__ bool tet_is_min(uint32_t k) { return k == 9u; }
__device__ __forceinline__ double obs_combine(double a, double b, uint32_t k, bool tets) {
    if (tets) return tet_is_min(k) ? fmin(a, b) : a + b;
    return k < 3u ? fmin(a, b) : fmax(a, b);
}
__device__ __forceinline__ double obs_identity(uint32_t k, bool tets) {
    if (tets) return tet_is_min(k) ? INFINITY : 0.0;
    return k < 3u ? INFINITY : k < 6u ? -INFINITY : 0.0;
}

// The fixed tree of a workgroup of 256: wave64 shuffles (lane l takes lane l + 32, 16, .. 1), then the four waves' results through LDS
// as (w0 + w1) + (w2 + w3).  The result is valid in thread 0.  Counts travel as integers.
template <uint32_t K, bool TETS, class Count>
__device__ __forceinline__ void obs_block_reduce(double (&v)[K], Count& n, double (*lds)[kObsTetVals], unsigned long long* lds_n) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t off = 32u; off; off >>= 1) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) v[k] = obs_combine(v[k], __shfl_down(v[k], off), k, TETS);
        n += __shfl_down(n, off);
    }
    __syncthreads();   // (the LDS rows may still be read by the reduction before this one)
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) lds[wave][k] = v[k];
        lds_n[wave] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++)
            v[k] = obs_combine(obs_combine(lds[0][k], lds[1][k], k, TETS), obs_combine(lds[2][k], lds[3][k], k, TETS), k, TETS);
        n = static_cast<Count>((lds_n[0] + lds_n[1]) + (lds_n[2] + lds_n[3]));
    }
}

// First launch: one workgroup per chunk, one lane per tet / particle; the chunk's partial row leaves through thread 0.
__global__ __launch_bounds__(256) void observe_chunks_kernel(const ObsChunk* __restrict__ chunks, const int4* __restrict__ tets, const double* __restrict__ v0,
                                                            const float4* __restrict__ pos, const float4* __restrict__ vel, const uint32_t* __restrict__ map,
                                                            double density, double* __restrict__ partial) {
    __shared__ double lds[4][kObsTetVals];
    __shared__ unsigned long long lds_n[4];
    const ObsChunk c = chunks[blockIdx.x];
    double* const row = partial + static_cast<uint64_t>(blockIdx.x) * kObsPartial;
    const bool live = threadIdx.x < c.count;
    const uint32_t r = c.first + threadIdx.x;
    if (c.kind == kObsTets) {
        double v[kObsTetVals];
#pragma unroll
        for (uint32_t k = 0; k < kObsTetVals; k++) v[k] = obs_identity(k, true);
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
        obs_block_reduce<kObsTetVals, true>(v, inverted, lds, lds_n);
        if (threadIdx.x == 0u) {
#pragma unroll
            for (uint32_t k = 0; k < kObsTetVals; k++) row[k] = v[k];
            row[kTetCountAt] = __longlong_as_double(static_cast<long long>(inverted));
            row[11] = 0.0;
        }
    } else {
        double v[kObsVertVals];
#pragma unroll
        for (uint32_t k = 0; k < kObsVertVals; k++) v[k] = obs_identity(k, false);
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
        obs_block_reduce<kObsVertVals, false>(v, nonfinite, lds, lds_n);
        if (threadIdx.x == 0u) {
#pragma unroll
            for (uint32_t k = 0; k < kObsVertVals; k++) row[k] = v[k];
            row[kVertCountAt] = __longlong_as_double(static_cast<long long>(nonfinite));
#pragma unroll
            for (uint32_t k = kVertCountAt + 1u; k < kObsPartial; k++) row[k] = 0.0;
        }
    }
}

// Second launch: one workgroup per body.  Thread t folds the body's partial rows t, t + 256, .. in that order, then the same tree; thread 0
// divides and stores the finished row.
__global__ __launch_bounds__(256) void observe_finish_kernel(const ObsBody* __restrict__ bodies, const double* __restrict__ partial, char* __restrict__ dst, uint64_t stride) {
    __shared__ double lds[4][kObsTetVals];
    __shared__ unsigned long long lds_n[4];
    const ObsBody b = bodies[blockIdx.x];
    double t[kObsTetVals], p[kObsVertVals];
    unsigned long long inverted = 0ull, nonfinite = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < kObsTetVals; k++) t[k] = obs_identity(k, true);
#pragma unroll
    for (uint32_t k = 0; k < kObsVertVals; k++) p[k] = obs_identity(k, false);
    for (uint32_t j = threadIdx.x; j < b.tet_chunks; j += 256u) {
        const double* const row = partial + static_cast<uint64_t>(b.tet_chunk0 + j) * kObsPartial;
#pragma unroll
        for (uint32_t k = 0; k < kObsTetVals; k++) t[k] = obs_combine(t[k], row[k], k, true);
        inverted += static_cast<unsigned long long>(__double_as_longlong(row[kTetCountAt]));
    }
    for (uint32_t j = threadIdx.x; j < b.vert_chunks; j += 256u) {
        const double* const row = partial + static_cast<uint64_t>(b.vert_chunk0 + j) * kObsPartial;
#pragma unroll
        for (uint32_t k = 0; k < kObsVertVals; k++) p[k] = obs_combine(p[k], row[k], k, false);
        nonfinite += static_cast<unsigned long long>(__double_as_longlong(row[kVertCountAt]));
    }
    obs_block_reduce<kObsTetVals, true>(t, inverted, lds, lds_n);
    obs_block_reduce<kObsVertVals, false>(p, nonfinite, lds, lds_n);
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

// The constant tables, built and uploaded by the handle's first observation (the only part of a call that blocks, with the export's
// events and index map): per tet its four API particle ids and V0, per chunk its body and rows, per body its chunks; and the scratch
// of the partial rows and the rows of the host read.  All of it counts into TetSimInfo.device_bytes from then on.
int ensure_tables(tetsim_body* h) {
    ObsDev& d = h->obs;
    if (d.ready) return 0;
    const uint32_t nt = h->info.num_elems;
    std::vector<uint32_t> fv, ft;
    body_ranges(h, &fv, &ft);
    const uint32_t nb = static_cast<uint32_t>(fv.size() - 1);
    std::vector<int4> ids(nt);
    std::vector<double> v0(nt);
    for (uint32_t e = 0; e < nt; e++) {
        const int32_t* t = &h->h_tets[4ull * e];
        ids[e] = make_int4(t[0], t[1], t[2], t[3]);
        v0[e] = rest_volume(h->h_verts.data(), t);   // (body.h)
    }
    std::vector<ObsChunk> chunks;
    std::vector<ObsBody> bodies(nb);
    auto cut = [&](uint32_t body, uint32_t first, uint32_t end, uint32_t kind) {
        for (uint32_t at = first; at < end; at += kObsChunk) chunks.push_back({body, at, std::min(kObsChunk, end - at), kind});
    };
    for (uint32_t b = 0; b < nb; b++) {
        bodies[b].tet_chunk0 = static_cast<uint32_t>(chunks.size());
        cut(b, ft[b], ft[b + 1], kObsTets);
        bodies[b].tet_chunks = static_cast<uint32_t>(chunks.size()) - bodies[b].tet_chunk0;
    }
    for (uint32_t b = 0; b < nb; b++) {
        bodies[b].vert_chunk0 = static_cast<uint32_t>(chunks.size());
        cut(b, fv[b], fv[b + 1], kObsVerts);
        bodies[b].vert_chunks = static_cast<uint32_t>(chunks.size()) - bodies[b].vert_chunk0;
    }
    int4* d_ids = nullptr; double* d_v0 = nullptr; ObsChunk* d_chunks = nullptr; ObsBody* d_bodies = nullptr;
    if (int rc = dev_alloc(h, &d_ids, ids.size())) return rc;
    if (int rc = dev_alloc(h, &d_v0, v0.size())) return rc;
    if (int rc = dev_alloc(h, &d_chunks, chunks.size())) return rc;
    if (int rc = dev_alloc(h, &d_bodies, bodies.size())) return rc;
    if (int rc = dev_alloc(h, &d.partial, chunks.size() * kObsPartial)) return rc;
    if (int rc = dev_alloc(h, &d.rows, static_cast<size_t>(nb) * TETSIM_OBS_WIDTH)) return rc;
    if (int rc = upload(h, d_ids, ids)) return rc;
    if (int rc = upload(h, d_v0, v0)) return rc;
    if (int rc = upload(h, d_chunks, chunks)) return rc;
    if (int rc = upload(h, d_bodies, bodies)) return rc;
    d.tets = d_ids; d.v0 = d_v0; d.chunks = d_chunks; d.bodies = d_bodies;
    d.n_chunks = static_cast<uint32_t>(chunks.size());
    d.ready = true;   // (last: set only when every table is there)
    return 0;
}

// the two launches on h->stream: row b of dst = body b
int enqueue_observation(tetsim_body* h, void* dst, uint64_t stride) {
    const ObsDev& d = h->obs;
    FieldSrc src[2];
    std::string why;
    if (int rc = resolve_field(h, TETSIM_FIELD_POSITIONS, false, &src[0], &why)) return fail(h, rc, why);
    if (int rc = resolve_field(h, TETSIM_FIELD_VELOCITIES, false, &src[1], &why)) return fail(h, rc, why);
    if (int rc = prepare_fields(h, src, 2)) return rc;
    if (d.n_chunks)
        hipLaunchKernelGGL(observe_chunks_kernel, dim3(d.n_chunks), dim3(256), 0, h->stream, static_cast<const ObsChunk*>(d.chunks), static_cast<const int4*>(d.tets), d.v0,
                           src[0].src, src[1].src, src[0].mapped ? h->d_api2dev : nullptr, h->opt.density, d.partial);
    if (int rc = launched(h)) return rc;
    hipLaunchKernelGGL(observe_finish_kernel, dim3(h->info.num_bodies), dim3(256), 0, h->stream, static_cast<const ObsBody*>(d.bodies), static_cast<const double*>(d.partial),
                       static_cast<char*>(dst), stride);
    return launched(h);
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_observe_bodies_device(tetsim_handle h, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!dst) return fail(h, TETSIM_EINVAL, "dst is null");
    if (reinterpret_cast<uintptr_t>(dst) % 8) return fail(h, TETSIM_EINVAL, "dst is not 8-byte aligned");
    constexpr uint64_t row = 8ull * TETSIM_OBS_WIDTH;
    if (row_stride != 0 && (row_stride < row || row_stride % 8)) return fail(h, TETSIM_EINVAL, "row_stride must be 0 or a multiple of 8 of at least 160");
    if (int rc = device_call_guard(h)) return rc;
    const uint64_t stride = row_stride ? row_stride : row;
    const uint32_t nb = h->info.num_bodies;
    if (int rc = check_device_span(h, dst, static_cast<uint64_t>(nb - 1u) * stride + row, "dst", std::to_string(nb) + " rows do not fit the allocation it points into")) return rc;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_tables(h)) return rc;
    return on_caller_stream(h, caller_stream, [&] { return enqueue_observation(h, dst, stride); });
}

int tetsim_read_body_observations(tetsim_handle h, double* out) {
    if (!h) return TETSIM_EINVAL;
    if (!out) return fail(h, TETSIM_EINVAL, "out is null");
    if (int rc = device_call_guard(h)) return rc;
    if (int rc = ensure_tables(h)) return rc;
    if (int rc = enqueue_observation(h, h->obs.rows, 8ull * TETSIM_OBS_WIDTH)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->obs.rows, static_cast<size_t>(h->info.num_bodies) * TETSIM_OBS_WIDTH * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
