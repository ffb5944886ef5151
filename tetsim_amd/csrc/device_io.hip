// device_io.hip -- how rows of the state leave the device arrays on the device: what a TETSIM_FIELD_* is on this body
// (resolve_field), what has to run before it is read (prepare_fields), ONE gather kernel.  The pinned reads and the visual mesh's reads
// (tetsim_state.hip, tetsim_visual.hip) gather into the handle's staging buffer; C ABI, part 5 (include/tetsim.h) -- tetsim_export_device / tetsim_import_device -- hands the same rows to another GPU program
// in ITS device memory, ordered against ITS stream, with no host copy and no host synchronisation.  See body.h.
#include "body.h"

using namespace tetsim;

namespace tetsim {
namespace {

// One field of a gather: row r = 3 or 4 floats of src[map ? map[r] : r] at dst + r * stride.  The table travels by value.
struct IoField {
    const float4* src;
    const uint32_t* map;      // API row -> device index, null = identity
    char* dst;
    uint64_t stride;          // bytes
    uint32_t rows, width;     // width: floats per row
    uint32_t first_block, pad;
};
struct IoTable {
    IoField f[TETSIM_MAX_EXPORT_FIELDS];
    uint32_t count, pad;
};
static_assert(sizeof(IoTable) <= 512, "the export table is a kernel argument");

// A lane = one row of one field (the fields' blocks follow each other in the grid): one 16-byte load through the index map, 3 or 4
// dword stores -- the destination is only 4-byte aligned and its rows may be padded, and nothing but the payload is written.
__global__ __launch_bounds__(256) void export_kernel(IoTable t) {
    uint32_t k = 0;
    while (k + 1u < t.count && blockIdx.x >= t.f[k + 1u].first_block) k++;   // (uniform: scalar loads from the argument segment)
    const IoField& f = t.f[k];
    const uint32_t r = (blockIdx.x - f.first_block) * 256u + threadIdx.x;
    if (r >= f.rows) return;
    const float4 p = f.src[f.map ? f.map[r] : r];
    float* const o = reinterpret_cast<float*>(f.dst + static_cast<uint64_t>(r) * f.stride);
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    if (f.width == 4u) o[3] = p.w;
}

// tetsim_write_state on the device (tetsim_import_device): API particle a -> device slot map[a].  p0 = end-of-substep positions; p1 = the polar solver's
// predictions (null for Neo-Hookean, whose position keeps its inverse mass in w).
__global__ __launch_bounds__(256) void import_kernel(const char* __restrict__ pos, uint64_t pos_stride, const char* __restrict__ vel, uint64_t vel_stride,
                                                     const uint32_t* __restrict__ map, uint32_t n, float4* __restrict__ p0, float4* __restrict__ p1,
                                                     float4* __restrict__ v) {
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= n) return;
    const float* const ps = reinterpret_cast<const float*>(pos + static_cast<uint64_t>(a) * pos_stride);
    const float* const vs = reinterpret_cast<const float*>(vel + static_cast<uint64_t>(a) * vel_stride);
    const uint32_t dv = map ? map[a] : a;
    const float4 p = make_float4(ps[0], ps[1], ps[2], p1 ? 0.0f : p0[dv].w);
    p0[dv] = p;
    if (p1) p1[dv] = p;
    v[dv] = make_float4(vs[0], vs[1], vs[2], 0.0f);
}

// the gather on h->stream: row r of field k to dst[k] + r * stride[k]; a field without a dst is left out
int gather(tetsim_body* h, const FieldSrc* s, void* const* dst, const uint64_t* stride, uint32_t count) {
    IoTable t{};
    uint32_t blocks = 0;
    for (uint32_t k = 0; k < count; k++) {
        t.f[k] = {s[k].src, s[k].mapped ? h->d_api2dev : nullptr, static_cast<char*>(dst[k]), stride[k], dst[k] ? s[k].rows : 0u, s[k].width, blocks, 0u};
        blocks += (t.f[k].rows + 255u) / 256u;
    }
    t.count = count;
    if (blocks) hipLaunchKernelGGL(export_kernel, dim3(blocks), dim3(256), 0, h->stream, t);
    return launched(h);
}

// rows of `width` floats: the general checks below with 4-byte units
bool stride_ok(uint64_t stride, uint32_t width) { return record_stride_ok(stride, 4ull * width, 4u); }
int check_device_rows(tetsim_body* h, const void* ptr, uint64_t stride, uint32_t rows, uint32_t width, const std::string& what) {
    return check_device_records(h, ptr, stride, rows, 4ull * width, 4u, what);
}

}  // namespace

bool record_stride_ok(uint64_t stride, uint64_t row_bytes, uint32_t align) { return stride == 0 || (stride >= row_bytes && stride % align == 0); }
int check_device_records(tetsim_body* h, const void* ptr, uint64_t stride, uint32_t rows, uint64_t row_bytes, uint32_t align, const std::string& what) {
    if (!ptr) return fail(h, TETSIM_EINVAL, what + " is null");
    if (reinterpret_cast<uintptr_t>(ptr) % align) return fail(h, TETSIM_EINVAL, what + " is not " + std::to_string(align) + "-byte aligned");
    return check_device_span(h, ptr, rows ? static_cast<uint64_t>(rows - 1u) * stride + row_bytes : 0u, what,
                             std::to_string(rows) + " rows do not fit the allocation it points into");
}

const char* const kPartitionedIo = "device export / import of a partitioned body is not supported (its halo stream and its ghosts need a contract of their own)";

int device_call_guard(tetsim_body* h) {
    if (h->partitioned) return fail(h, TETSIM_ESTATE, kPartitionedIo);
    HIPCHK(h, hipSetDevice(h->opt.device));
    return 0;
}
int launched(tetsim_body* h) {
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? 0 : fail(h, TETSIM_EHIP, std::string("kernel launch: ") + hipGetErrorString(le));
}
int check_device_span(tetsim_body* h, const void* ptr, uint64_t need, const std::string& what, const std::string& misfit) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, TETSIM_EINVAL, what + " is not device memory (hipPointerGetAttributes does not know it)");
    }
    if (at.type != hipMemoryTypeDevice || at.device != h->opt.device)
        return fail(h, TETSIM_EINVAL, what + " is not device memory of device " + std::to_string(h->opt.device));
    if (need == 0) return 0;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(ptr)) != hipSuccess) { (void)hipGetLastError(); return 0; }   // (no extent on record: the type check stands)
    const uint64_t off = reinterpret_cast<uintptr_t>(ptr) - reinterpret_cast<uintptr_t>(base);
    if (off > size || need > size - off) return fail(h, TETSIM_EINVAL, what + ": " + misfit);
    return 0;
}
// the two events of this call, the first recorded on the caller's stream and awaited by the handle's
int io_begin(tetsim_body* h, hipStream_t caller, hipEvent_t** ev) {
    for (auto& pair : h->ev_io)
        for (hipEvent_t& e : pair)
            if (!e) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *ev = h->ev_io[h->io_parity++ & 1u];
    HIPCHK(h, hipEventRecord((*ev)[0], caller));
    HIPCHK(h, hipStreamWaitEvent(h->stream, (*ev)[0], 0));
    return 0;
}
int io_end(tetsim_body* h, hipStream_t caller, hipEvent_t* ev) {
    HIPCHK(h, hipEventRecord(ev[1], h->stream));
    HIPCHK(h, hipStreamWaitEvent(caller, ev[1], 0));
    return 0;
}

int drain(tetsim_body* h) {
    HIPCHK(h, hipSetDevice(h->opt.device));
    if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
    return 0;
}

// include/tetsim.h defines every TETSIM_FIELD_* as "what tetsim_read_X returns": this is that definition.  The host readers are older
// than the export and word three refusals in their own way (host_reader); both wordings are what callers match on.
int resolve_field(tetsim_body* h, int32_t field, bool host_reader, FieldSrc* f, std::string* why) {
    const bool pjs = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI;
    const bool has_map = pjs && !h->api2dev.empty();   // (only the polar solver renumbers its particles)
    const uint32_t nv = h->info.owned_particles;
    auto refuse = [&](int code, const std::string& msg) { *why = msg; return code; };
    *f = FieldSrc{};
    switch (field) {
        case TETSIM_FIELD_POSITIONS: f->src = current_positions(h); f->rows = nv; f->mapped = has_map; return 0;
        case TETSIM_FIELD_VELOCITIES: f->src = pjs ? h->pj.vel : h->nh.vel; f->rows = nv; f->mapped = has_map; return 0;
        case TETSIM_FIELD_PREV_POSITIONS:
            // (tetsim_read_prev_positions names the reader, the export the field)
            if (pjs) return refuse(TETSIM_ESTATE, std::string("POLAR_JACOBI does not keep prevPos after a substep (it equals the previous ") + (host_reader ? "read_positions)" : "positions)"));
            f->src = h->nh.prev; f->rows = nv;
            return 0;
        case TETSIM_FIELD_QUATS:   // rows in tetsim_get_local_tets order: the array's own
            if (!pjs) return refuse(TETSIM_ESTATE, "quaternions exist only for POLAR_JACOBI");
            f->src = h->pj.quat; f->rows = h->pj.nt; f->width = 4u; f->quats = true;
            return 0;
        case TETSIM_FIELD_VISUAL_POSITIONS:
        case TETSIM_FIELD_VISUAL_NORMALS:
        case TETSIM_FIELD_VISUAL_VERTEX_NORMALS: {
            const SkinDev& k = h->skin;
            const bool vnrm = field == TETSIM_FIELD_VISUAL_VERTEX_NORMALS;
            // (tetsim_read_visual_vertex_normals / _from never looked at vis_attached: without a mesh they miss the TRIANGLES, below)
            if (!h->vis_attached && !(host_reader && vnrm)) return refuse(TETSIM_ESTATE, "no visual mesh attached (tetsim_set_visual_mesh)");
            // (tetsim_read_visual_mesh never looked at the solver: a Neo-Hookean body with an EMPTY visual mesh may ask it for normals)
            if (field == TETSIM_FIELD_VISUAL_NORMALS && ((!pjs && !host_reader) || (k.nvis && !k.out_nrm)))
                return refuse(TETSIM_ESTATE, "normals need POLAR_JACOBI and rest normals at tetsim_set_visual_mesh");
            if (vnrm && !k.vt_off) return refuse(TETSIM_ESTATE, "no visual triangles attached (tetsim_set_visual_triangles)");
            f->src = field == TETSIM_FIELD_VISUAL_POSITIONS ? k.out_pos : vnrm ? k.out_vnrm : k.out_nrm;
            f->rows = k.nvis;
            f->skin = true;
            f->quats = pjs;   // (the skinning kernel rotates the rest normals by the tets' quaternions)
            f->vnrm = vnrm;
            return 0;
        }
        default: return refuse(TETSIM_EINVAL, "unknown field");
    }
}

int prepare_fields(tetsim_body* h, const FieldSrc* f, uint32_t count) {
    bool map = false, quats = false, skin = false, vnrm = false;
    for (uint32_t k = 0; k < count; k++) { map |= f[k].mapped; quats |= f[k].quats; skin |= f[k].skin; vnrm |= f[k].vnrm; }
    if (skin && h->partitioned && !h->neigh.empty() && !h->final_ghosts_fresh)
        // The corners this partition does not own: their end-of-substep positions come from the neighbours, by an EXPLICIT call every rank
        // makes.  (Round 5 ran the RCCL exchange from inside this read, gated by a per-rank flag: one rank reading twice per frame, or only
        // some ranks having refreshed, left the others alone inside a collective -- a hang.  A read never communicates.)
        return fail(h, TETSIM_ESTATE, "the ghost particles' end-of-substep positions are stale: after the frame's last substep every rank calls tetsim_halo_refresh_final "
                                      "(RCCL; in-process groups: tetsim_group_refresh_final) before it reads the visual mesh of a partition");
    if (map) { if (int rc = ensure_index_map(h)) return rc; }
    if (quats) { if (int rc = ensure_quats(h)) return rc; }
    if (skin) {   // Softbody.js arithmetic for the solver that mirrors Softbody.js, the vertex-shader arithmetic for the other (SoftbodyGPU.js:440 reads the quaternions)
        const bool pjs = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI;
        skin_launch(h->stream, h->skin, pjs ? h->pj.pos_final : h->nh.pos, pjs ? h->pj.quat : nullptr, !pjs);
        if (vnrm) skin_launch_vertex_normals(h->stream, h->skin);
    }
    return 0;
}

int read_rows(tetsim_body* h, const FieldSrc* f, float* const* out, uint32_t count, bool pinned) {
    // the gather packs the fields into the staging buffer one after the other; rows that are in the caller's format already (the
    // quaternions) are copied straight from their array
    void* at[TETSIM_MAX_EXPORT_FIELDS] = {};
    uint64_t stride[TETSIM_MAX_EXPORT_FIELDS];
    auto staged = [&](uint32_t k) { return f[k].width == 3u || f[k].mapped ? static_cast<size_t>(f[k].rows) * f[k].width : 0; };   // floats
    size_t floats = 0;
    for (uint32_t k = 0; k < count; k++) floats += staged(k);
    if (floats) { if (int rc = dev_grow(h, &h->d_packed, &h->packed_cap, floats)) return rc; }
    float* p = h->d_packed;
    for (uint32_t k = 0; k < count; k++) {
        stride[k] = 4ull * f[k].width;
        if (staged(k)) at[k] = p;
        p += staged(k);
    }
    if (int rc = gather(h, f, at, stride, count)) return rc;
    if (!pinned) HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint32_t k = 0; k < count; k++) {
        const void* from = at[k] ? at[k] : f[k].src;
        const size_t bytes = f[k].rows * stride[k];
        if (bytes && pinned) HIPCHK(h, hipMemcpyAsync(out[k], from, bytes, hipMemcpyDeviceToHost, h->stream));
        else if (bytes) HIPCHK(h, hipMemcpy(out[k], from, bytes, hipMemcpyDeviceToHost));
    }
    if (pinned) HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int read_fields(tetsim_body* h, const FieldSrc* f, float* const* out, uint32_t count, bool pinned) {
    HIPCHK(h, hipSetDevice(h->opt.device));
    if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));   // (the halo queue's tiles write particles and quaternions too)
    if (int rc = prepare_fields(h, f, count)) return rc;
    return read_rows(h, f, out, count, pinned);
}

}  // namespace tetsim

extern "C" {

int tetsim_export_device(tetsim_handle h, const TetSimDeviceField* fields, uint32_t count, void* consumer_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!fields) return fail(h, TETSIM_EINVAL, "fields is null");
    if (count == 0 || count > TETSIM_MAX_EXPORT_FIELDS) return fail(h, TETSIM_EINVAL, "count must be 1 .. TETSIM_MAX_EXPORT_FIELDS");
    if (int rc = device_call_guard(h)) return rc;
    FieldSrc src[TETSIM_MAX_EXPORT_FIELDS];
    void* dst[TETSIM_MAX_EXPORT_FIELDS];
    uint64_t stride[TETSIM_MAX_EXPORT_FIELDS];
    for (uint32_t k = 0; k < count; k++) {
        const TetSimDeviceField& in = fields[k];
        const std::string at = "field " + std::to_string(k) + ": ";
        std::string why;
        if (in.reserved != 0) return fail(h, TETSIM_EINVAL, at + "reserved must be 0");
        if (int rc = resolve_field(h, in.field, false, &src[k], &why)) return fail(h, rc, at + why);
        if (!stride_ok(in.row_stride, src[k].width)) return fail(h, TETSIM_EINVAL, at + "row_stride must be 0 or a multiple of 4 of at least the row's bytes");
        stride[k] = in.row_stride ? in.row_stride : 4ull * src[k].width;
        if (int rc = check_device_rows(h, dst[k] = in.dst, stride[k], src[k].rows, src[k].width, at + "dst")) return rc;
    }
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    return on_caller_stream(h, consumer_stream, [&]() -> int {
        if (int rc = prepare_fields(h, src, count)) return rc;
        return gather(h, src, dst, stride, count);
    });
}

int tetsim_import_device(tetsim_handle h, const void* pos, uint64_t pos_stride, const void* vel, uint64_t vel_stride, void* producer_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!pos || !vel) return fail(h, TETSIM_EINVAL, "null argument");
    if (h->partitioned) return fail(h, TETSIM_ESTATE, kPartitionedIo);   // (device_call_guard's two steps, with the stride check between them as ever)
    if (!stride_ok(pos_stride, 3u) || !stride_ok(vel_stride, 3u)) return fail(h, TETSIM_EINVAL, "a stride must be 0 or a multiple of 4 of at least 12");
    HIPCHK(h, hipSetDevice(h->opt.device));
    const uint32_t n = h->info.owned_particles;
    const uint64_t ps = pos_stride ? pos_stride : 12u, vs = vel_stride ? vel_stride : 12u;
    if (int rc = check_device_rows(h, pos, ps, n, 3u, "pos")) return rc;
    if (int rc = check_device_rows(h, vel, vs, n, 3u, "vel")) return rc;
    return on_caller_stream(h, producer_stream, [&]() -> int {
        const bool pjs = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI, mapped = pjs && !h->api2dev.empty();
        if (mapped) { if (int rc = ensure_index_map(h)) return rc; }
        if (n) hipLaunchKernelGGL(import_kernel, dim3((n + 255u) / 256u), dim3(256), 0, h->stream, static_cast<const char*>(pos), ps, static_cast<const char*>(vel), vs,
                                  mapped ? h->d_api2dev : nullptr, n, pjs ? h->pj.pos_final : h->nh.pos, pjs ? h->pj.pos_pred : nullptr, pjs ? h->pj.vel : h->nh.vel);
        if (int rc = launched(h)) return rc;
        if (pjs) {
            h->pred_any_dt = false;
            h->dt_pred = std::nanf("");  // forces a re-prediction at the next step
        }
        return 0;
    });
}

}  // extern "C"
