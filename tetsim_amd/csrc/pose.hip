// pose.hip -- C ABI, per-body pose (include/tetsim.h): tetsim_body_poses_device / tetsim_read_body_poses.  One row of TETSIM_POSE_WIDTH
// doubles per body of the handle: the mass moments of the current positions and velocities against a constant per-particle table (lumped
// mass, rest position about the rest mass centre), and what follows from them -- mass centre and its velocity, the best-fit rotation
// (Horn's quaternion: a fixed number of cyclic Jacobi sweeps on a symmetric 4x4), angular velocity and momentum about the mass centre, the
// rms distance to the best rigid fit.  Positions and velocities come from the rows the export hands out (device_io.hip: resolve_field /
// prepare_fields, gathered through d_api2dev), and the call is ordered against the caller's stream as the observation is
// (on_caller_stream).  f64 arithmetic, every operation rounded on its own (this unit is built with -ffp-contract=off); the fixed reduction
// tree of body_reduce.h over the body's particle chunks, no atomics: the same state gives the same bits, and a body of a batch the bits
// it gives alone.  The derived values use only + - * / sqrt on the stored raw values: tests/pose_ref.py gives the same bits in numpy.
// See body.h.
#include "body_reduce.h"

using namespace tetsim;

namespace tetsim {
namespace {

constexpr uint32_t kRaw = 26;           // the raw moments: row values [0..25], and a chunk's partial row; every one a sum
constexpr uint32_t kSweeps = TETSIM_POSE_SWEEPS;   // cyclic Jacobi sweeps (include/tetsim.h says why)
static_assert(TETSIM_POSE_COM == kRaw, "the derived values follow the raw moments");

// First launch: one workgroup per chunk, one lane per particle; the chunk's 26 sums leave through thread 0.
__global__ __launch_bounds__(256) void pose_chunks_kernel(const BodyChunk* __restrict__ chunks, const PoseRec* __restrict__ table, const float4* __restrict__ pos,
                                                         const float4* __restrict__ vel, const uint32_t* __restrict__ map, double* __restrict__ partial) {
    __shared__ double lds[4][kRaw];
    const BodyChunk c = chunks[blockIdx.x];
    double v[kRaw];
#pragma unroll
    for (uint32_t k = 0; k < kRaw; k++) v[k] = 0.0;
    if (threadIdx.x < c.count) {
        const uint32_t r = c.first + threadIdx.x;
        const double2* const rec = reinterpret_cast<const double2*>(table + r);   // { m, qx } { qy, qz }: two 16-byte loads
        const double2 mq0 = rec[0], mq1 = rec[1];
        const uint32_t i = map ? map[r] : r;
        const float4 xf = pos[i], uf = vel[i];
        const double m = mq0.x, q[3] = {mq0.y, mq1.x, mq1.y};
        const double x[3] = {xf.x, xf.y, xf.z}, u[3] = {uf.x, uf.y, uf.z};
        double mx[3];
        v[TETSIM_POSE_MASS] = m;
#pragma unroll
        for (uint32_t a = 0; a < 3u; a++) {
            mx[a] = m * x[a];
            v[TETSIM_POSE_MX + a] = mx[a];
            v[TETSIM_POSE_MV + a] = m * u[a];
#pragma unroll
            for (uint32_t b = 0; b < 3u; b++) v[TETSIM_POSE_A + 3u * a + b] = mx[a] * q[b];
        }
        v[TETSIM_POSE_L0] = m * (x[1] * u[2] - x[2] * u[1]);
        v[TETSIM_POSE_L0 + 1] = m * (x[2] * u[0] - x[0] * u[2]);
        v[TETSIM_POSE_L0 + 2] = m * (x[0] * u[1] - x[1] * u[0]);
        v[TETSIM_POSE_G] = mx[0] * x[0];
        v[TETSIM_POSE_G + 1] = mx[1] * x[1];
        v[TETSIM_POSE_G + 2] = mx[2] * x[2];
        v[TETSIM_POSE_G + 3] = mx[0] * x[1];
        v[TETSIM_POSE_G + 4] = mx[0] * x[2];
        v[TETSIM_POSE_G + 5] = mx[1] * x[2];
        v[TETSIM_POSE_Q0] = m * ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    }
    block_reduce<SumOps>(v, lds);
    if (threadIdx.x == 0u) {
        double* const row = partial + static_cast<uint64_t>(blockIdx.x) * kRaw;
#pragma unroll
        for (uint32_t k = 0; k < kRaw; k++) row[k] = v[k];
    }
}

// One Jacobi rotation of the pair (P, Q) of the symmetric 4x4 n (both triangles kept) with the eigenvectors e: the strain section's
// formulas.  N_pq == 0 leaves everything as it is (a NaN is not 0: the rotation runs and the NaN spreads).
template <uint32_t P, uint32_t Q>
__device__ __forceinline__ void pose_rotate(double (&n)[4][4], double (&e)[4][4]) {
    const double pq = n[P][Q];
    if (pq == 0.0) return;
    const double pp = n[P][P], qq = n[Q][Q];
    const double theta = (qq - pp) / (2.0 * pq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tpq = t * pq;
    n[P][P] = pp - tpq;
    n[Q][Q] = qq + tpq;
    n[P][Q] = n[Q][P] = 0.0;
#pragma unroll
    for (uint32_t r = 0; r < 4u; r++) {
        if (r != P && r != Q) {
            const double rp = n[r][P], rq = n[r][Q];
            n[r][P] = n[P][r] = c * rp - s * rq;
            n[r][Q] = n[Q][r] = s * rp + c * rq;
        }
        const double ep = e[r][P], eq = e[r][Q];
        e[r][P] = c * ep - s * eq;
        e[r][Q] = s * ep + c * eq;
    }
}

// The derived values [26..47] of a row from its stored raw values [0..25] (include/tetsim.h, THE ROW, PART 2), expression for expression.
__device__ __forceinline__ void pose_derive(double* __restrict__ o) {
#pragma unroll
    for (uint32_t k = kRaw; k < TETSIM_POSE_WIDTH; k++) o[k] = 0.0;
    o[TETSIM_POSE_Q + 3] = 1.0;
    const double mass = o[TETSIM_POSE_MASS];
    if (mass == 0.0) return;
    const double mx[3] = {o[TETSIM_POSE_MX], o[TETSIM_POSE_MX + 1], o[TETSIM_POSE_MX + 2]};
    const double mv[3] = {o[TETSIM_POSE_MV], o[TETSIM_POSE_MV + 1], o[TETSIM_POSE_MV + 2]};
    double com[3];
#pragma unroll
    for (uint32_t a = 0; a < 3u; a++) {
        com[a] = mx[a] / mass;
        o[TETSIM_POSE_COM + a] = com[a];
        o[TETSIM_POSE_VCOM + a] = mv[a] / mass;
    }
    const double lx = o[TETSIM_POSE_L0] - (com[1] * mv[2] - com[2] * mv[1]);
    const double ly = o[TETSIM_POSE_L0 + 1] - (com[2] * mv[0] - com[0] * mv[2]);
    const double lz = o[TETSIM_POSE_L0 + 2] - (com[0] * mv[1] - com[1] * mv[0]);
    o[TETSIM_POSE_L] = lx; o[TETSIM_POSE_L + 1] = ly; o[TETSIM_POSE_L + 2] = lz;
    const double gxx = o[TETSIM_POSE_G] - (mx[0] * mx[0]) / mass, gyy = o[TETSIM_POSE_G + 1] - (mx[1] * mx[1]) / mass;
    const double gzz = o[TETSIM_POSE_G + 2] - (mx[2] * mx[2]) / mass, gxy = o[TETSIM_POSE_G + 3] - (mx[0] * mx[1]) / mass;
    const double gxz = o[TETSIM_POSE_G + 4] - (mx[0] * mx[2]) / mass, gyz = o[TETSIM_POSE_G + 5] - (mx[1] * mx[2]) / mass;
    const double tr = (gxx + gyy) + gzz;
    const double ixx = tr - gxx, iyy = tr - gyy, izz = tr - gzz, ixy = -gxy, ixz = -gxz, iyz = -gyz;
    const double a00 = iyy * izz - iyz * iyz, a01 = ixz * iyz - ixy * izz, a02 = ixy * iyz - ixz * iyy;
    const double a11 = ixx * izz - ixz * ixz, a12 = ixy * ixz - ixx * iyz, a22 = ixx * iyy - ixy * ixy;
    const double det = (ixx * a00 + ixy * a01) + ixz * a02;
    if (det != 0.0) {   // (a NaN is not 0: it divides and spreads)
        o[TETSIM_POSE_OMEGA] = ((a00 * lx + a01 * ly) + a02 * lz) / det;
        o[TETSIM_POSE_OMEGA + 1] = ((a01 * lx + a11 * ly) + a12 * lz) / det;
        o[TETSIM_POSE_OMEGA + 2] = ((a02 * lx + a12 * ly) + a22 * lz) / det;
    }
    // S_ab = A_ba
    const double* const A = o + TETSIM_POSE_A;
    const double sxx = A[0], syx = A[1], szx = A[2], sxy = A[3], syy = A[4], szy = A[5], sxz = A[6], syz = A[7], szz = A[8];
    double n[4][4], e[4][4];
    n[0][0] = (sxx + syy) + szz;
    n[1][1] = (sxx - syy) - szz;
    n[2][2] = (syy - sxx) - szz;
    n[3][3] = (szz - sxx) - syy;
    n[0][1] = n[1][0] = syz - szy;
    n[0][2] = n[2][0] = szx - sxz;
    n[0][3] = n[3][0] = sxy - syx;
    n[1][2] = n[2][1] = sxy + syx;
    n[1][3] = n[3][1] = szx + sxz;
    n[2][3] = n[3][2] = syz + szy;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++)
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) e[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (uint32_t sweep = 0; sweep < kSweeps; sweep++) {
        pose_rotate<0, 1>(n, e);
        pose_rotate<0, 2>(n, e);
        pose_rotate<0, 3>(n, e);
        pose_rotate<1, 2>(n, e);
        pose_rotate<1, 3>(n, e);
        pose_rotate<2, 3>(n, e);
    }
    // the largest diagonal entry, ties to the lower index (a NaN leaves 0); its column; the largest of the other three
    uint32_t kmax = 0u;
    double lam = n[0][0];
#pragma unroll
    for (uint32_t k = 1; k < 4u; k++) {
        const bool better = n[k][k] > lam;
        lam = better ? n[k][k] : lam;
        kmax = better ? k : kmax;
    }
    double w = e[0][0], x = e[1][0], y = e[2][0], z = e[3][0];
#pragma unroll
    for (uint32_t k = 1; k < 4u; k++) {
        const bool pick = k == kmax;
        w = pick ? e[0][k] : w; x = pick ? e[1][k] : x; y = pick ? e[2][k] : y; z = pick ? e[3][k] : z;
    }
    double second = kmax == 0u ? n[1][1] : n[0][0];
#pragma unroll
    for (uint32_t k = 1; k < 4u; k++) {
        const bool take = k != kmax && n[k][k] > second;
        second = take ? n[k][k] : second;
    }
    const double len = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / len; x = x / len; y = y / len; z = z / len;
    const double first = x != 0.0 ? x : (y != 0.0 ? y : z);   // the first non-zero of x, y, z (or z == 0)
    const bool flip = w < 0.0 || (w == 0.0 && first < 0.0);
    o[TETSIM_POSE_Q] = flip ? -x : x;
    o[TETSIM_POSE_Q + 1] = flip ? -y : y;
    o[TETSIM_POSE_Q + 2] = flip ? -z : z;
    o[TETSIM_POSE_Q + 3] = flip ? -w : w;
    const double res = ((tr + o[TETSIM_POSE_Q0]) - 2.0 * lam) / mass;
    o[TETSIM_POSE_RESIDUAL] = sqrt(res < 0.0 ? 0.0 : res);
    o[TETSIM_POSE_GAP] = lam - second;
}

// Second launch: one workgroup per body.  The fold of the body's chunk rows (body_reduce.h: fold_rows), then the same tree; thread 0
// stores the raw values, runs the derived procedure on the values it just stored, and stores the rest.
__global__ __launch_bounds__(256) void pose_finish_kernel(const BodyChunks* __restrict__ bodies, const double* __restrict__ partial, char* __restrict__ dst, uint64_t stride) {
    __shared__ double lds[4][kRaw];
    double v[kRaw];
    fold_rows<SumOps, kRaw>(bodies[blockIdx.x], partial, v);
    block_reduce<SumOps>(v, lds);
    if (threadIdx.x != 0u) return;
    double o[TETSIM_POSE_WIDTH];
#pragma unroll
    for (uint32_t k = 0; k < kRaw; k++) o[k] = v[k];
    pose_derive(o);
    double* const out = reinterpret_cast<double*>(dst + static_cast<uint64_t>(blockIdx.x) * stride);
#pragma unroll
    for (uint32_t k = 0; k < TETSIM_POSE_WIDTH; k++) out[k] = o[k];
}

// What the handle's first pose call builds and uploads (the only part of a call that blocks, with the export's events and index map): the
// particle chunk table (body_reduce.h) unless another call made it, per particle its record, the scratch of the chunk rows and the rows
// of the host read.  All of it counts into TetSimInfo.device_bytes from then on.
int ensure_tables(tetsim_body* h) {
    PoseDev& d = h->pose;
    if (d.ready) return 0;
    if (int rc = ensure_chunk_table(h, kParticleChunks)) return rc;
    const uint32_t nt = h->info.num_elems, nv = h->info.num_particles;
    std::vector<uint32_t> fv, ft;
    body_ranges(h, &fv, &ft);
    const uint32_t nb = static_cast<uint32_t>(fv.size() - 1);
    std::vector<PoseRec> recs(nv);
    build_pose_table(h->h_verts.data(), nv, h->h_tets.data(), nt, fv.data(), nb, h->opt.density, recs.data(), nullptr);
    PoseRec* d_recs = nullptr;
    if (int rc = dev_alloc(h, &d_recs, recs.size())) return rc;
    if (int rc = dev_alloc(h, &d.partial, static_cast<size_t>(h->chunk_table[kParticleChunks].n_chunks) * kRaw)) return rc;
    if (int rc = dev_alloc(h, &d.rows, static_cast<size_t>(nb) * TETSIM_POSE_WIDTH)) return rc;
    if (int rc = upload(h, d_recs, recs)) return rc;
    d.table = d_recs;
    d.ready = true;   // (last: set only when every table is there)
    return 0;
}

// the two launches on h->stream: row b of dst = body b
int enqueue_poses(tetsim_body* h, void* dst, uint64_t stride) {
    const PoseDev& d = h->pose;
    const ChunkTable& t = h->chunk_table[kParticleChunks];
    FieldSrc src[2];
    if (int rc = export_sources(h, {TETSIM_FIELD_POSITIONS, TETSIM_FIELD_VELOCITIES}, src)) return rc;
    if (t.n_chunks)
        hipLaunchKernelGGL(pose_chunks_kernel, dim3(t.n_chunks), dim3(256), 0, h->stream, t.chunks, static_cast<const PoseRec*>(d.table),
                           src[0].src, src[1].src, src[0].mapped ? h->d_api2dev : nullptr, d.partial);
    if (int rc = launched(h)) return rc;
    hipLaunchKernelGGL(pose_finish_kernel, dim3(h->info.num_bodies), dim3(256), 0, h->stream, t.bodies, static_cast<const double*>(d.partial), static_cast<char*>(dst), stride);
    return launched(h);
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_body_poses_device(tetsim_handle h, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    uint64_t stride;
    if (int rc = check_dst_rows(h, dst, row_stride, h->info.num_bodies, 8ull * TETSIM_POSE_WIDTH, 8u, &stride)) return rc;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_tables(h)) return rc;
    return on_caller_stream(h, caller_stream, [&] { return enqueue_poses(h, dst, stride); });
}

int tetsim_read_body_poses(tetsim_handle h, double* out) {
    if (!h) return TETSIM_EINVAL;
    if (!out) return fail(h, TETSIM_EINVAL, "out is null");
    if (int rc = device_call_guard(h)) return rc;
    if (int rc = ensure_tables(h)) return rc;
    return read_back(h, out, h->pose.rows, static_cast<size_t>(h->info.num_bodies) * TETSIM_POSE_WIDTH, [&] { return enqueue_poses(h, h->pose.rows, 8ull * TETSIM_POSE_WIDTH); });
}

}  // extern "C"
