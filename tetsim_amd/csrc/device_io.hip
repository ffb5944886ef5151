// device_io.hip -- C ABI, part 5 (include/tetsim.h): the state handed to / taken from another GPU program in ITS device memory, ordered
// against ITS stream -- no host copy, no host synchronisation.  The producing kernels are the ones the host reads use (lean-state
// quaternion recovery, skinning, vertex normals); what is here is the last hop -- one gather kernel out, one scatter kernel in -- and
// the stream contract around it.  See body.h.
#include "body.h"

using namespace tetsim;

namespace tetsim {
namespace {

// One field of an export: row r = 3 or 4 floats of src[map ? map[r] : r] at dst + r * stride.  The table travels by value.
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

// tetsim_write_state on the device: API particle a -> device slot map[a].  p0 = end-of-substep positions; p1 = the polar solver's
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

// 0 = packed; else at least the row and a multiple of 4
bool stride_ok(uint64_t stride, uint32_t width) { return stride == 0 || (stride >= 4ull * width && stride % 4 == 0); }

// `ptr` is device memory of the handle's device, 4-byte aligned, and `rows` rows of `width` floats `stride` bytes apart fit the allocation
int check_device_rows(tetsim_body* h, const void* ptr, uint64_t stride, uint32_t rows, uint32_t width, const std::string& what) {
    if (!ptr) return fail(h, TETSIM_EINVAL, what + " is null");
    if (reinterpret_cast<uintptr_t>(ptr) % 4) return fail(h, TETSIM_EINVAL, what + " is not 4-byte aligned");
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, TETSIM_EINVAL, what + " is not device memory (hipPointerGetAttributes does not know it)");
    }
    if (at.type != hipMemoryTypeDevice || at.device != h->opt.device)
        return fail(h, TETSIM_EINVAL, what + " is not device memory of device " + std::to_string(h->opt.device));
    if (rows == 0) return 0;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(ptr)) != hipSuccess) { (void)hipGetLastError(); return 0; }   // (no extent on record: the type check stands)
    const uint64_t off = reinterpret_cast<uintptr_t>(ptr) - reinterpret_cast<uintptr_t>(base);
    const uint64_t need = static_cast<uint64_t>(rows - 1u) * stride + 4ull * width;
    if (off > size || need > size - off) return fail(h, TETSIM_EINVAL, what + ": " + std::to_string(rows) + " rows do not fit the allocation it points into");
    return 0;
}

const char* const kPartitionedIo = "device export / import of a partitioned body is not supported (its halo stream and its ghosts need a contract of their own)";

int ensure_io_events(tetsim_body* h) {
    for (auto& pair : h->ev_io)
        for (hipEvent_t& ev : pair)
            if (!ev) HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return 0;
}

}  // namespace
}  // namespace tetsim

extern "C" {

int tetsim_export_device(tetsim_handle h, const TetSimDeviceField* fields, uint32_t count, void* consumer_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!fields) return fail(h, TETSIM_EINVAL, "fields is null");
    if (count == 0 || count > TETSIM_MAX_EXPORT_FIELDS) return fail(h, TETSIM_EINVAL, "count must be 1 .. TETSIM_MAX_EXPORT_FIELDS");
    if (h->partitioned) return fail(h, TETSIM_ESTATE, kPartitionedIo);
    HIPCHK(h, hipSetDevice(h->opt.device));
    const bool pjs = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI;
    const uint32_t nv = h->info.owned_particles, nvis = h->skin.nvis;
    IoTable t{};
    const bool has_map = pjs && !h->api2dev.empty();   // (as the host reads: only the polar solver renumbers its particles)
    bool need_quats = false, need_skin = false, need_vnrm = false, need_map = false;
    bool mapped[TETSIM_MAX_EXPORT_FIELDS] = {};
    uint32_t blocks = 0;
    for (uint32_t k = 0; k < count; k++) {
        const TetSimDeviceField& in = fields[k];
        const std::string at = "field " + std::to_string(k) + ": ";
        if (in.reserved != 0) return fail(h, TETSIM_EINVAL, at + "reserved must be 0");
        IoField& f = t.f[k];
        f.width = 3u;
        switch (in.field) {
            case TETSIM_FIELD_POSITIONS: f.src = current_positions(h); f.rows = nv; mapped[k] = has_map; break;
            case TETSIM_FIELD_VELOCITIES: f.src = pjs ? h->pj.vel : h->nh.vel; f.rows = nv; mapped[k] = has_map; break;
            case TETSIM_FIELD_PREV_POSITIONS:
                if (pjs) return fail(h, TETSIM_ESTATE, at + "POLAR_JACOBI does not keep prevPos after a substep (it equals the previous positions)");
                f.src = h->nh.prev; f.rows = nv;
                break;
            case TETSIM_FIELD_QUATS:
                if (!pjs) return fail(h, TETSIM_ESTATE, at + "quaternions exist only for POLAR_JACOBI");
                f.src = h->pj.quat; f.rows = h->pj.nt; f.width = 4u; need_quats = true;
                break;
            case TETSIM_FIELD_VISUAL_POSITIONS:
            case TETSIM_FIELD_VISUAL_NORMALS:
            case TETSIM_FIELD_VISUAL_VERTEX_NORMALS:
                if (!h->vis_attached) return fail(h, TETSIM_ESTATE, at + "no visual mesh attached (tetsim_set_visual_mesh)");
                if (in.field == TETSIM_FIELD_VISUAL_NORMALS && (!pjs || (nvis && !h->skin.out_nrm)))
                    return fail(h, TETSIM_ESTATE, at + "normals need POLAR_JACOBI and rest normals at tetsim_set_visual_mesh");
                if (in.field == TETSIM_FIELD_VISUAL_VERTEX_NORMALS && !h->skin.vt_off)
                    return fail(h, TETSIM_ESTATE, at + "no visual triangles attached (tetsim_set_visual_triangles)");
                f.src = in.field == TETSIM_FIELD_VISUAL_POSITIONS ? h->skin.out_pos : in.field == TETSIM_FIELD_VISUAL_NORMALS ? h->skin.out_nrm : h->skin.out_vnrm;
                f.rows = nvis;
                need_skin = true;
                need_quats = need_quats || pjs;   // (the skinning kernel rotates the rest normals by the tets' quaternions)
                need_vnrm = need_vnrm || in.field == TETSIM_FIELD_VISUAL_VERTEX_NORMALS;
                break;
            default: return fail(h, TETSIM_EINVAL, at + "unknown field");
        }
        if (!stride_ok(in.row_stride, f.width)) return fail(h, TETSIM_EINVAL, at + "row_stride must be 0 or a multiple of 4 of at least the row's bytes");
        f.stride = in.row_stride ? in.row_stride : 4ull * f.width;
        if (int rc = check_device_rows(h, in.dst, f.stride, f.rows, f.width, at + "dst")) return rc;
        f.dst = static_cast<char*>(in.dst);
        need_map = need_map || mapped[k];
        f.first_block = blocks;
        blocks += (f.rows + 255u) / 256u;
    }
    t.count = count;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (need_map) { if (int rc = ensure_index_map(h)) return rc; }
    for (uint32_t k = 0; k < count; k++) if (mapped[k]) t.f[k].map = h->d_api2dev;
    if (int rc = ensure_io_events(h)) return rc;
    hipStream_t const cs = static_cast<hipStream_t>(consumer_stream);
    hipEvent_t* const ev = h->ev_io[h->io_parity++ & 1u];
    HIPCHK(h, hipEventRecord(ev[0], cs));
    HIPCHK(h, hipStreamWaitEvent(h->stream, ev[0], 0));
    if (need_quats) { if (int rc = ensure_quats(h)) return rc; }
    if (need_skin) {   // Softbody.js arithmetic for the solver that mirrors Softbody.js, the vertex-shader arithmetic for the other (tetsim_read_visual_mesh)
        skin_launch(h->stream, h->skin, pjs ? h->pj.pos_final : h->nh.pos, pjs ? h->pj.quat : nullptr, !pjs);
        if (need_vnrm) skin_launch_vertex_normals(h->stream, h->skin);
    }
    if (blocks) hipLaunchKernelGGL(export_kernel, dim3(blocks), dim3(256), 0, h->stream, t);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(h, TETSIM_EHIP, std::string("kernel launch: ") + hipGetErrorString(le));
    HIPCHK(h, hipEventRecord(ev[1], h->stream));
    HIPCHK(h, hipStreamWaitEvent(cs, ev[1], 0));
    return 0;
}

int tetsim_import_device(tetsim_handle h, const void* pos, uint64_t pos_stride, const void* vel, uint64_t vel_stride, void* producer_stream) {
    if (!h) return TETSIM_EINVAL;
    if (!pos || !vel) return fail(h, TETSIM_EINVAL, "null argument");
    if (h->partitioned) return fail(h, TETSIM_ESTATE, kPartitionedIo);
    if (!stride_ok(pos_stride, 3u) || !stride_ok(vel_stride, 3u)) return fail(h, TETSIM_EINVAL, "a stride must be 0 or a multiple of 4 of at least 12");
    HIPCHK(h, hipSetDevice(h->opt.device));
    const bool pjs = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI;
    const uint32_t n = h->info.owned_particles;
    const uint64_t ps = pos_stride ? pos_stride : 12u, vs = vel_stride ? vel_stride : 12u;
    if (int rc = check_device_rows(h, pos, ps, n, 3u, "pos")) return rc;
    if (int rc = check_device_rows(h, vel, vs, n, 3u, "vel")) return rc;
    const bool mapped = pjs && !h->api2dev.empty();
    if (mapped) { if (int rc = ensure_index_map(h)) return rc; }
    if (int rc = ensure_io_events(h)) return rc;
    hipStream_t const ps_ = static_cast<hipStream_t>(producer_stream);
    hipEvent_t* const ev = h->ev_io[h->io_parity++ & 1u];
    HIPCHK(h, hipEventRecord(ev[0], ps_));
    HIPCHK(h, hipStreamWaitEvent(h->stream, ev[0], 0));
    if (n) hipLaunchKernelGGL(import_kernel, dim3((n + 255u) / 256u), dim3(256), 0, h->stream, static_cast<const char*>(pos), ps, static_cast<const char*>(vel), vs,
                              mapped ? h->d_api2dev : nullptr, n, pjs ? h->pj.pos_final : h->nh.pos, pjs ? h->pj.pos_pred : nullptr, pjs ? h->pj.vel : h->nh.vel);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(h, TETSIM_EHIP, std::string("kernel launch: ") + hipGetErrorString(le));
    HIPCHK(h, hipEventRecord(ev[1], h->stream));
    HIPCHK(h, hipStreamWaitEvent(ps_, ev[1], 0));
    if (pjs) {
        h->pred_any_dt = false;
        h->dt_pred = std::nanf("");  // forces a re-prediction at the next step
    }
    return 0;
}

}  // extern "C"
