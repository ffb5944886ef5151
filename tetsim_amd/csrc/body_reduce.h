// body_reduce.h -- what the per-body device calls share (observe.hip, strain.hip, pose.hip, body_grabs.hip): the cut of every body into
// chunks of 256 rows counted from ITS first particle / tet, the fixed reduction tree of a workgroup of 256, the fold of a body's chunk rows,
// and the host steps around them.  The public header's promise -- the same state gives the same bits, and a body of a batch the bits it
// gives alone -- rests on the cut and the tree being one thing: no atomics, nothing that depends on where a body sits in a batch.
#pragma once
#include <type_traits>

#include "body_rows.h"

namespace tetsim {

constexpr uint32_t kBodyChunk = 256;    // rows of one workgroup
struct BodyChunk { uint32_t first, count, body; };   // first: the chunk's first particle / tet in the API's numbering
struct BodyChunks { uint32_t chunk0, chunks; };      // a body's chunks: their range in the table, so also its partial rows

struct NoCount {};                      // a reduction without an integer count
struct SumOps {                         // every value a sum
    static __device__ __forceinline__ double combine(double a, double b, uint32_t) { return a + b; }
    static __device__ __forceinline__ double identity(uint32_t) { return 0.0; }
};

// The fixed tree of a workgroup of 256 over K values, Ops::combine(a, b, k) / Ops::identity(k) per value: wave64 shuffles (lane l takes
// lane l + 32, 16, .. 1), then lane 0 of the four waves through LDS, one barrier, thread 0 combines (w0, w1) with (w2, w3).  The result is
// valid in thread 0.  A count (anything but NoCount) travels as an integer.  A kernel that reduces twice through the same LDS rows puts
// its own barrier between the two.
template <class Ops, uint32_t K, uint32_t S, class Count>
__device__ __forceinline__ void block_reduce(double (&v)[K], Count& n, double (&lds)[4][S], unsigned long long (&lds_n)[4]) {
    static_assert(K <= S, "the LDS rows hold the values");
    constexpr bool counted = !std::is_same<Count, NoCount>::value;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t off = 32u; off; off >>= 1) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) v[k] = Ops::combine(v[k], __shfl_down(v[k], off), k);
        if constexpr (counted) n += __shfl_down(n, off);
    }
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) lds[wave][k] = v[k];
        if constexpr (counted) lds_n[wave] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < K; k++) v[k] = Ops::combine(Ops::combine(lds[0][k], lds[1][k], k), Ops::combine(lds[2][k], lds[3][k], k), k);
        if constexpr (counted) n = static_cast<Count>((lds_n[0] + lds_n[1]) + (lds_n[2] + lds_n[3]));
    }
}
template <class Ops, uint32_t K>
__device__ __forceinline__ void block_reduce(double (&v)[K], double (&lds)[4][K]) {
    NoCount none;
    unsigned long long unused[4];
    block_reduce<Ops>(v, none, lds, unused);
}

// A finish kernel's start: thread t folds the body's partial rows t, t + 256, .. in that order, from the identities.  rows: the first
// partial row of the table the body's chunks count in, W doubles each; a count sits at [count_at] as a 64-bit integer in the double's place.
template <class Ops, uint32_t W, uint32_t K, class Count>
__device__ __forceinline__ void fold_rows(const BodyChunks& b, const double* __restrict__ rows, double (&v)[K], Count& n, uint32_t count_at) {
    constexpr bool counted = !std::is_same<Count, NoCount>::value;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) v[k] = Ops::identity(k);
    for (uint32_t j = threadIdx.x; j < b.chunks; j += kBodyChunk) {
        const double* const row = rows + static_cast<uint64_t>(b.chunk0 + j) * W;
#pragma unroll
        for (uint32_t k = 0; k < K; k++) v[k] = Ops::combine(v[k], row[k], k);
        if constexpr (counted) n += static_cast<Count>(__double_as_longlong(row[count_at]));
    }
}
template <class Ops, uint32_t W, uint32_t K>
__device__ __forceinline__ void fold_rows(const BodyChunks& b, const double* __restrict__ rows, double (&v)[K]) {
    NoCount none;
    fold_rows<Ops, W>(b, rows, v, none, 0u);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// The handle's chunk table over its particles or over its tets, cut on the host and uploaded by whichever call needs it first (the only
// part of such a call that blocks, with its own constant table, the export's events and index map); it counts into
// TetSimInfo.device_bytes from then on.
inline int ensure_chunk_table(tetsim_body* h, ChunkKind kind) {
    ChunkTable& t = h->chunk_table[kind];
    if (t.chunks) return 0;
    std::vector<uint32_t> first_vert, first_tet;
    body_ranges(h, &first_vert, &first_tet);
    const std::vector<uint32_t>& first = kind == kTetChunks ? first_tet : first_vert;
    std::vector<BodyChunk> chunks;
    std::vector<BodyChunks> bodies(first.size() - 1);
    for (uint32_t b = 0; b < bodies.size(); b++) {
        bodies[b].chunk0 = static_cast<uint32_t>(chunks.size());
        for (uint32_t at = first[b]; at < first[b + 1]; at += kBodyChunk) chunks.push_back({at, std::min(kBodyChunk, first[b + 1] - at), b});
        bodies[b].chunks = static_cast<uint32_t>(chunks.size()) - bodies[b].chunk0;
    }
    BodyChunk* d_chunks = nullptr; BodyChunks* d_bodies = nullptr;
    if (int rc = dev_alloc(h, &d_chunks, chunks.size())) return rc;
    if (int rc = dev_alloc(h, &d_bodies, bodies.size())) return rc;
    if (int rc = upload(h, d_chunks, chunks)) return rc;
    if (int rc = upload(h, d_bodies, bodies)) return rc;
    t.bodies = d_bodies;
    t.n_chunks = static_cast<uint32_t>(chunks.size());
    t.chunks = d_chunks;   // (last: set only when the table is there)
    return 0;
}

// The checks of a destination of `rows` records in the caller's device memory, in every call's order: dst, the stride, the handle's guard,
// then the records (device_io.hip: check_device_records).  *stride: the resolved stride.
inline int check_dst_rows(tetsim_body* h, const void* dst, uint64_t row_stride, uint32_t rows, uint64_t row_bytes, uint32_t align, uint64_t* stride) {
    if (!dst) return fail(h, TETSIM_EINVAL, "dst is null");
    if (int rc = check_record_stride(h, "row_stride", row_stride, row_bytes, align)) return rc;
    if (int rc = device_call_guard(h)) return rc;
    *stride = resolved_stride(row_stride, row_bytes);
    return check_device_records(h, dst, *stride, rows, row_bytes, align, "dst");
}

// the fields as the export hands them out (device_io.hip), prepared on h->stream
template <uint32_t N>
inline int export_sources(tetsim_body* h, const int32_t (&fields)[N], FieldSrc (&src)[N]) {
    std::string why;
    for (uint32_t k = 0; k < N; k++)
        if (int rc = resolve_field(h, fields[k], false, &src[k], &why)) return fail(h, rc, why);
    return prepare_fields(h, src, N);
}

// the tail of a host read: what `enqueue` puts on h->stream writes the handle's own `rows`; they reach `out` behind a stream sync
template <class T, class F>
inline int read_back(tetsim_body* h, T* out, const T* rows, size_t count, F&& enqueue) {
    if (int rc = enqueue()) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, rows, count * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace tetsim
