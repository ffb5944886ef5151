// strain.hip -- C ABI, part 9 (include/tetsim.h): tetsim_tet_strain_device / tetsim_read_tet_strain / tetsim_body_strain_device /
// tetsim_visual_strain_device.  Per tet the deformation gradient F = P * invRestPose, its determinant, the reference's r_s, the principal
// stretches (a fixed number of cyclic Jacobi sweeps on C = F^T F) and the norm of the Green strain; per body their extremes and a
// volume-weighted sum; per visual row one channel of its tet.  Positions come from the rows the export hands out (device_io.hip:
// resolve_field / prepare_fields, gathered through d_api2dev), so no stepping path's tet order matters, and the calls are ordered against
// the caller's stream as the export is (on_caller_stream).  f64 arithmetic on the stored f32 values with only + - * / sqrt, every
// operation rounded on its own (this unit is built with -ffp-contract=off): tests/strain_ref.py gives the same bits in numpy.  The body
// row is reduced by the fixed tree of body_reduce.h over its tet chunks, no atomics.  See body.h.
#include "body_reduce.h"

using namespace tetsim;

namespace tetsim {
namespace {

constexpr uint32_t kChunk = kBodyChunk; // tets of one workgroup
constexpr uint32_t kSweeps = TETSIM_STRAIN_SWEEPS;   // cyclic Jacobi sweeps (include/tetsim.h says why 4)
constexpr uint32_t kVals = 15;          // values of a tet row (RESERVED is the 16th float)
constexpr uint32_t kBodyVals = 7;       // reduced floating-point values of a body row; the count travels as an integer
constexpr uint32_t kLdsRow = 20;        // floats between two staged rows: 16 + 4, so that the lanes' 16-byte writes spread over the banks

enum : uint32_t { kRowsNone = 0u, kRowsPlain = 1u, kRowsStaged = 2u };

__device__ __forceinline__ StrainRec load_rec(const StrainRec* __restrict__ table, uint32_t r) {
    union { uint4 q[4]; StrainRec rec; } u;
    const uint4* const p = reinterpret_cast<const uint4*>(table + r);
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) u.q[k] = p[k];
    return u.rec;
}

// one Jacobi rotation of the pair (p, q) of a symmetric 3x3; rp / rq: the third index's entries.  C_pq == 0 leaves everything as it is
// (a NaN is not 0: the rotation runs and the NaN spreads); selects, not branches: every lane does the same work.
__device__ __forceinline__ void jacobi_rotate(double& pp, double& qq, double& pq, double& rp, double& rq) {
    const bool skip = pq == 0.0;
    const double theta = (qq - pp) / (2.0 * pq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tpq = t * pq;
    const double npp = pp - tpq, nqq = qq + tpq, nrp = c * rp - s * rq, nrq = s * rp + c * rq;
    pp = skip ? pp : npp;
    qq = skip ? qq : nqq;
    rp = skip ? rp : nrp;
    rq = skip ? rq : nrq;
    pq = skip ? pq : 0.0;
}

// The 15 values of a tet in f64 (include/tetsim.h, DEFINITIONS).  A degenerate tet gives NaN everywhere.
__device__ __forceinline__ void strain_of(const StrainRec& rec, const float4* __restrict__ pos, const uint32_t* __restrict__ map, double (&v)[kVals]) {
    const uint32_t i0 = map ? map[rec.id[0]] : rec.id[0], i1 = map ? map[rec.id[1]] : rec.id[1];
    const uint32_t i2 = map ? map[rec.id[2]] : rec.id[2], i3 = map ? map[rec.id[3]] : rec.id[3];
    const float4 x0 = pos[i0], x1 = pos[i1], x2 = pos[i2], x3 = pos[i3];
    // P_ik = x_{k+1}[i] - x_0[i]
    const double p[3][3] = {{static_cast<double>(x1.x) - x0.x, static_cast<double>(x2.x) - x0.x, static_cast<double>(x3.x) - x0.x},
                            {static_cast<double>(x1.y) - x0.y, static_cast<double>(x2.y) - x0.y, static_cast<double>(x3.y) - x0.y},
                            {static_cast<double>(x1.z) - x0.z, static_cast<double>(x2.z) - x0.z, static_cast<double>(x3.z) - x0.z}};
    double f[3][3];   // f[i][j] = F_ij
#pragma unroll
    for (uint32_t j = 0; j < 3u; j++) {
        const double b0 = rec.b[3u * j], b1 = rec.b[3u * j + 1u], b2 = rec.b[3u * j + 2u];
#pragma unroll
        for (uint32_t i = 0; i < 3u; i++) {
            f[i][j] = (p[i][0] * b0 + p[i][1] * b1) + p[i][2] * b2;
            v[TETSIM_STRAIN_F + 3u * j + i] = f[i][j];
        }
    }
    v[TETSIM_STRAIN_J] = (f[0][0] * (f[1][1] * f[2][2] - f[1][2] * f[2][1]) - f[0][1] * (f[1][0] * f[2][2] - f[1][2] * f[2][0])) +
                         f[0][2] * (f[1][0] * f[2][1] - f[1][1] * f[2][0]);
    // C = F^T F, each pair once
    double c00 = (f[0][0] * f[0][0] + f[1][0] * f[1][0]) + f[2][0] * f[2][0];
    double c01 = (f[0][0] * f[0][1] + f[1][0] * f[1][1]) + f[2][0] * f[2][1];
    double c02 = (f[0][0] * f[0][2] + f[1][0] * f[1][2]) + f[2][0] * f[2][2];
    double c11 = (f[0][1] * f[0][1] + f[1][1] * f[1][1]) + f[2][1] * f[2][1];
    double c12 = (f[0][1] * f[0][2] + f[1][1] * f[1][2]) + f[2][1] * f[2][2];
    double c22 = (f[0][2] * f[0][2] + f[1][2] * f[1][2]) + f[2][2] * f[2][2];
    v[TETSIM_STRAIN_DEV] = sqrt((c00 + c11) + c22);
    {
        const double e00 = (c00 - 1.0) / 2.0, e11 = (c11 - 1.0) / 2.0, e22 = (c22 - 1.0) / 2.0;
        const double e01 = c01 / 2.0, e02 = c02 / 2.0, e12 = c12 / 2.0;
        double g = e00 * e00;
        g = g + e11 * e11;
        g = g + e22 * e22;
        g = g + 2.0 * (e01 * e01);
        g = g + 2.0 * (e02 * e02);
        g = g + 2.0 * (e12 * e12);
        v[TETSIM_STRAIN_GREEN] = sqrt(g);
    }
#pragma unroll 1
    for (uint32_t sweep = 0; sweep < kSweeps; sweep++) {
        jacobi_rotate(c00, c11, c01, c02, c12);   // (0,1), third index 2
        jacobi_rotate(c00, c22, c02, c01, c12);   // (0,2), third index 1
        jacobi_rotate(c11, c22, c12, c01, c02);   // (1,2), third index 0
    }
    double s0 = sqrt(c00 < 0.0 ? 0.0 : c00), s1 = sqrt(c11 < 0.0 ? 0.0 : c11), s2 = sqrt(c22 < 0.0 ? 0.0 : c22);
    // descending: swap where the earlier one is smaller (a NaN stays where it is)
    { const bool w = s0 < s1; const double a = w ? s1 : s0, b = w ? s0 : s1; s0 = a; s1 = b; }
    { const bool w = s0 < s2; const double a = w ? s2 : s0, b = w ? s0 : s2; s0 = a; s2 = b; }
    { const bool w = s1 < s2; const double a = w ? s2 : s1, b = w ? s1 : s2; s1 = a; s2 = b; }
    v[TETSIM_STRAIN_STRETCH] = s0; v[TETSIM_STRAIN_STRETCH + 1] = s1; v[TETSIM_STRAIN_STRETCH + 2] = s2;
    if (rec.degenerate) {
#pragma unroll
        for (uint32_t k = 0; k < kVals; k++) v[k] = __builtin_nan("");
    }
}

// the body row's values: [0] max, [1] min, [2] min, [3] max, [4] max, [5] [6] sums
struct BodyOps {
    static __device__ __forceinline__ double combine(double a, double b, uint32_t k) {
        return (k == 1u || k == 2u) ? fmin(a, b) : (k == 0u || k == 3u || k == 4u) ? fmax(a, b) : a + b;
    }
    static __device__ __forceinline__ double identity(uint32_t k) {
        return (k == 1u || k == 2u) ? INFINITY : (k == 0u || k == 3u || k == 4u) ? -INFINITY : 0.0;
    }
};

// One workgroup per chunk, one lane per tet.  rows: kRowsStaged -- rows are 64 bytes apart and dst is 16-byte aligned: the chunk's rows
// pass through LDS and leave as 16-byte stores that cover contiguous memory wave by wave; kRowsPlain -- 16 dword stores per row (the
// destination is only 4-byte aligned and its rows may be padded); kRowsNone -- no rows.  partial != null: the chunk's partial body row
// (7 doubles and the count of the tets left out) leaves through thread 0.
__global__ __launch_bounds__(256) void strain_chunks_kernel(const BodyChunk* __restrict__ chunks, const StrainRec* __restrict__ table, const float4* __restrict__ pos,
                                                           const uint32_t* __restrict__ map, char* __restrict__ dst, uint64_t stride, uint32_t rows,
                                                           double* __restrict__ partial) {
    __shared__ float4 staged[kChunk * kLdsRow / 4u];
    __shared__ double lds[4][kBodyVals];
    __shared__ unsigned long long lds_n[4];
    const BodyChunk c = chunks[blockIdx.x];
    const bool live = threadIdx.x < c.count;
    const uint32_t r = c.first + threadIdx.x;
    double b[kBodyVals];
#pragma unroll
    for (uint32_t k = 0; k < kBodyVals; k++) b[k] = BodyOps::identity(k);
    unsigned long long left_out = 0ull;
    if (live) {
        const StrainRec rec = load_rec(table, r);
        double v[kVals];
        strain_of(rec, pos, map, v);
        float o[TETSIM_STRAIN_WIDTH];
        bool finite = true;
#pragma unroll
        for (uint32_t k = 0; k < kVals; k++) {
            o[k] = static_cast<float>(v[k]);
            finite = finite && isfinite(o[k]);
        }
        o[TETSIM_STRAIN_RESERVED] = 0.0f;
        if (rows == kRowsStaged) {
            float4* const s = staged + threadIdx.x * (kLdsRow / 4u);
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) s[k] = make_float4(o[4u * k], o[4u * k + 1u], o[4u * k + 2u], o[4u * k + 3u]);
        } else if (rows == kRowsPlain) {
            float* const out = reinterpret_cast<float*>(dst + static_cast<uint64_t>(r) * stride);
#pragma unroll
            for (uint32_t k = 0; k < TETSIM_STRAIN_WIDTH; k++) out[k] = o[k];
        }
        if (finite && !rec.degenerate) {
            const double g = v[TETSIM_STRAIN_GREEN];
            b[0] = v[TETSIM_STRAIN_STRETCH]; b[1] = v[TETSIM_STRAIN_STRETCH + 2];
            b[2] = b[3] = v[TETSIM_STRAIN_J];
            b[4] = g;
            b[5] = rec.v0_abs * (g * g);
            b[6] = rec.v0_abs;
        } else left_out = 1ull;
    }
    if (rows == kRowsStaged) {   // (uniform)
        __syncthreads();
        // the chunk's rows are count * 64 contiguous bytes at dst + first * 64: 16-byte piece j = part j % 4 of row j / 4
        float4* const out = reinterpret_cast<float4*>(dst + static_cast<uint64_t>(c.first) * 64u);
        const uint32_t pieces = 4u * c.count;
#pragma unroll
        for (uint32_t j = threadIdx.x; j < 4u * kChunk; j += kChunk)
            if (j < pieces) out[j] = staged[(j >> 2) * (kLdsRow / 4u) + (j & 3u)];
    }
    if (!partial) return;   // (uniform)
    block_reduce<BodyOps>(b, left_out, lds, lds_n);
    if (threadIdx.x == 0u) {
        double* const row = partial + static_cast<uint64_t>(blockIdx.x) * TETSIM_STRAIN_BODY_WIDTH;
#pragma unroll
        for (uint32_t k = 0; k < kBodyVals; k++) row[k] = b[k];
        row[kBodyVals] = __longlong_as_double(static_cast<long long>(left_out));
    }
}

// One workgroup per body.  The fold of the body's partial rows (body_reduce.h: fold_rows), then the same tree; thread 0 stores the row.
__global__ __launch_bounds__(256) void strain_finish_kernel(const BodyChunks* __restrict__ bodies, const double* __restrict__ partial, char* __restrict__ dst, uint64_t stride) {
    __shared__ double lds[4][kBodyVals];
    __shared__ unsigned long long lds_n[4];
    double b[kBodyVals];
    unsigned long long left_out = 0ull;
    fold_rows<BodyOps, TETSIM_STRAIN_BODY_WIDTH>(bodies[blockIdx.x], partial, b, left_out, kBodyVals);
    block_reduce<BodyOps>(b, left_out, lds, lds_n);
    if (threadIdx.x != 0u) return;
    double* const o = reinterpret_cast<double*>(dst + static_cast<uint64_t>(blockIdx.x) * stride);
#pragma unroll
    for (uint32_t k = 0; k < kBodyVals; k++) o[k] = b[k];
    o[kBodyVals] = static_cast<double>(left_out);
}

// One lane per attached visual row: channel `channel` of the row's tet, the same arithmetic as the tet rows, one dword store.
__global__ __launch_bounds__(256) void strain_visual_kernel(const uint32_t* __restrict__ vis_tet, uint32_t nvis, const StrainRec* __restrict__ table, const float4* __restrict__ pos,
                                                           const uint32_t* __restrict__ map, uint32_t channel, char* __restrict__ dst, uint64_t stride) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= nvis) return;
    const StrainRec rec = load_rec(table, vis_tet[row]);
    double v[kVals];
    strain_of(rec, pos, map, v);
    double pick = v[0];
#pragma unroll
    for (uint32_t k = 1; k < kVals; k++) pick = k == channel ? v[k] : pick;
    *reinterpret_cast<float*>(dst + static_cast<uint64_t>(row) * stride) = static_cast<float>(pick);
}

// What the handle's first strain call builds and uploads (the only part of a call that blocks, with the export's events and index map):
// the tet chunk table (body_reduce.h) unless another call made it, per tet its record, the scratch of the partial rows and the rows of
// the host read.  All of it counts into TetSimInfo.device_bytes from then on.
int ensure_tables(tetsim_body* h) {
    StrainDev& d = h->strain;
    if (d.ready) return 0;
    if (int rc = ensure_chunk_table(h, kTetChunks)) return rc;
    const uint32_t nt = h->info.num_elems;
    std::vector<StrainRec> recs(nt);
    build_strain_table(h->h_verts.data(), h->info.num_particles, h->h_tets.data(), nt, h->opt.density, recs.data());
    StrainRec* d_recs = nullptr;
    if (int rc = dev_alloc(h, &d_recs, recs.size())) return rc;
    if (int rc = dev_alloc(h, &d.partial, static_cast<size_t>(h->chunk_table[kTetChunks].n_chunks) * TETSIM_STRAIN_BODY_WIDTH)) return rc;
    if (int rc = dev_alloc(h, &d.rows, static_cast<size_t>(nt) * TETSIM_STRAIN_WIDTH)) return rc;
    if (int rc = upload(h, d_recs, recs)) return rc;
    d.table = d_recs;
    d.ready = true;   // (last: set only when every table is there)
    return 0;
}

// the attached visual rows' tets, uploaded by the first tetsim_visual_strain_device
int ensure_visual_table(tetsim_body* h) {
    StrainDev& d = h->strain;
    if (d.vis_tet) return 0;
    uint32_t* p = nullptr;
    if (int rc = dev_alloc(h, &p, h->vis_tet.size())) return rc;
    if (int rc = upload(h, p, h->vis_tet)) return rc;
    d.vis_tet = p;
    return 0;
}

// the chunk launch on h->stream: tet rows to dst (or none), partial body rows (or none)
int enqueue_chunks(tetsim_body* h, void* dst, uint64_t stride, bool partial) {
    const StrainDev& d = h->strain;
    const ChunkTable& t = h->chunk_table[kTetChunks];
    if (!t.n_chunks) return 0;
    FieldSrc src[1];
    if (int rc = export_sources(h, {TETSIM_FIELD_POSITIONS}, src)) return rc;
    const uint32_t rows = !dst ? kRowsNone : (stride == 64u && reinterpret_cast<uintptr_t>(dst) % 16u == 0) ? kRowsStaged : kRowsPlain;
    hipLaunchKernelGGL(strain_chunks_kernel, dim3(t.n_chunks), dim3(256), 0, h->stream, t.chunks, static_cast<const StrainRec*>(d.table),
                       src[0].src, src[0].mapped ? h->d_api2dev : nullptr, static_cast<char*>(dst), stride, rows, partial ? d.partial : nullptr);
    return launched(h);
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_tet_strain_device(tetsim_handle h, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    uint64_t stride;
    if (int rc = check_dst_rows(h, dst, row_stride, h->info.num_elems, 4ull * TETSIM_STRAIN_WIDTH, 4u, &stride)) return rc;
    if (h->info.num_elems == 0) return 0;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_tables(h)) return rc;
    return on_caller_stream(h, caller_stream, [&] { return enqueue_chunks(h, dst, stride, false); });
}

int tetsim_read_tet_strain(tetsim_handle h, float* out) {
    if (!h) return TETSIM_EINVAL;
    if (!out) return fail(h, TETSIM_EINVAL, "out is null");
    if (int rc = device_call_guard(h)) return rc;
    if (h->info.num_elems == 0) return 0;
    if (int rc = ensure_tables(h)) return rc;
    return read_back(h, out, h->strain.rows, static_cast<size_t>(h->info.num_elems) * TETSIM_STRAIN_WIDTH, [&] { return enqueue_chunks(h, h->strain.rows, 4ull * TETSIM_STRAIN_WIDTH, false); });
}

int tetsim_body_strain_device(tetsim_handle h, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    uint64_t stride;
    if (int rc = check_dst_rows(h, dst, row_stride, h->info.num_bodies, 8ull * TETSIM_STRAIN_BODY_WIDTH, 8u, &stride)) return rc;
    if (int rc = ensure_tables(h)) return rc;
    return on_caller_stream(h, caller_stream, [&]() -> int {
        if (int rc = enqueue_chunks(h, nullptr, 0, true)) return rc;
        hipLaunchKernelGGL(strain_finish_kernel, dim3(h->info.num_bodies), dim3(256), 0, h->stream, h->chunk_table[kTetChunks].bodies,
                           static_cast<const double*>(h->strain.partial), static_cast<char*>(dst), stride);
        return launched(h);
    });
}

int tetsim_visual_strain_device(tetsim_handle h, int32_t channel, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!dst) return fail(h, TETSIM_EINVAL, "dst is null");
    if (channel < 0 || channel >= static_cast<int32_t>(TETSIM_STRAIN_RESERVED)) return fail(h, TETSIM_EINVAL, "channel must be one of 0..14 (TETSIM_STRAIN_*)");
    if (!record_stride_ok(row_stride, 4u, 4u)) return fail(h, TETSIM_EINVAL, "row_stride must be 0 or a multiple of 4");
    if (!h->vis_attached) return fail(h, TETSIM_ESTATE, "no visual mesh attached (tetsim_set_visual_mesh)");
    if (int rc = device_call_guard(h)) return rc;
    const uint64_t stride = row_stride ? row_stride : 4u;
    const uint32_t nvis = h->skin.nvis;
    if (int rc = check_device_records(h, dst, stride, nvis, 4u, 4u, "dst")) return rc;
    if (nvis == 0) return 0;
    if (int rc = ensure_tables(h)) return rc;
    if (int rc = ensure_visual_table(h)) return rc;
    return on_caller_stream(h, caller_stream, [&]() -> int {
        FieldSrc src[1];
        if (int rc = export_sources(h, {TETSIM_FIELD_POSITIONS}, src)) return rc;
        hipLaunchKernelGGL(strain_visual_kernel, dim3((nvis + 255u) / 256u), dim3(256), 0, h->stream, h->strain.vis_tet, nvis, static_cast<const StrainRec*>(h->strain.table),
                           src[0].src, src[0].mapped ? h->d_api2dev : nullptr, static_cast<uint32_t>(channel), static_cast<char*>(dst), stride);
        return launched(h);
    });
}

}  // extern "C"
