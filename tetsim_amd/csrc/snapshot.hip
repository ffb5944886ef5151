// snapshot.hip -- C ABI, part 6 (include/tetsim.h): tetsim_snapshot_*.  A snapshot is the handle's complete solver state in device memory -- one
// buffer per entry of state_sections() (tetsim_state.hip), what a checkpoint keeps on the host -- captured and restored for CHOSEN bodies of a
// batch by ONE copy kernel on the handle's stream, ordered against the caller's stream as the device export and import are (body.h:
// on_caller_stream).  The mask of the chosen bodies is device memory that the host never reads.  See body.h.
#include "body_rows.h"

using namespace tetsim;

struct tetsim_snapshot_s {
    tetsim_body* owner = nullptr;
    std::vector<void*> buf;        // one per state section, in state_sections() order
    std::vector<size_t> bytes;
    // for which dt the predictions in it are valid (tetsim_body::pred_any_dt / dt_pred at the captures, intersected)
    bool pred_any_dt = true;
    float dt_pred = 0.0f;
};

namespace tetsim {
namespace {

// How a row finds its body.  Particles, blocked tets (tetsim_create.hip: a body's particles keep their range in device numbering;
// host_prep.cpp: build_blocks sorts body after body and an unpartitioned body's tiles keep that order) and the gather path's tets (caller
// order) lie body after body: `table` = first row of every body, [bodies + 1]; a row at or behind table[bodies] is padding and belongs to no body
// (elem's planes are nt_pad rows long).  Neo-Hookean volError is indexed by the position in the solve sequence (nh_kernels.inc:
// vol_err[order[e]]; tetsim_create.hip: `pre`), and a coloured or clustered sequence interleaves the bodies: `table` = the body of every row.
enum : uint32_t { kRowsByRange = 0u, kRowsByTable = 1u };
struct SnapSection {
    char* dst;
    const char* src;
    const uint32_t* table;
    uint32_t rows, row_bytes;      // 16 (float4 sections), 8 (volError) or 4 (the lean state's ninth shape float)
    uint32_t first_block;
    uint32_t kind : 1, stamped : 1;   // stamped: the row's fourth float is a call's sequence number and leaves as 0 (tetsim_state.hip: clear_stamps)
};
constexpr uint32_t kMaxSnapSections = 8;
struct SnapTable {
    SnapSection s[kMaxSnapSections];
    const uint8_t* mask;           // [bodies] nonzero = chosen; null = every row, padding included
    uint32_t count, bodies;
};
static_assert(sizeof(SnapTable) <= 512, "the section table is a kernel argument");

// A workgroup moves a chunk of 1024 16-byte units of one section (the sections' chunks follow each other in the grid): four independent
// 16-byte loads per lane, consecutive lanes on consecutive units, then the four stores -- the shape of the streaming probe's copy
// (util_kernels.hip).  Every section starts on a 16-byte boundary (hipMalloc; elem's planes are nt_pad * 16 bytes apart), so a unit is
// 1, 2 or 4 whole rows; only a section's last unit can be short, and it moves row by row.
constexpr uint32_t kSnapLanes = 256, kSnapPerLane = 4, kSnapChunk = kSnapLanes * kSnapPerLane;

__device__ __forceinline__ uint32_t body_of_row(const uint32_t* __restrict__ first, uint32_t bodies, uint32_t row) {
    if (row >= first[bodies]) return bodies;   // padding
    uint32_t lo = 0, hi = bodies;              // first[lo] <= row < first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ bool row_chosen(const SnapSection& S, const uint8_t* __restrict__ mask, uint32_t bodies, uint32_t row) {
    const uint32_t b = S.kind == kRowsByTable ? S.table[row] : body_of_row(S.table, bodies, row);
    return b < bodies && mask[b] != 0;
}
__device__ __forceinline__ void move_row(const SnapSection& S, uint32_t row) {
    const uint64_t off = static_cast<uint64_t>(row) * S.row_bytes;
    if (S.row_bytes == 16u) {
        uint4 v = *reinterpret_cast<const uint4*>(S.src + off);
        if (S.stamped) v.w = 0u;
        *reinterpret_cast<uint4*>(S.dst + off) = v;
    } else if (S.row_bytes == 8u) *reinterpret_cast<uint2*>(S.dst + off) = *reinterpret_cast<const uint2*>(S.src + off);
    else *reinterpret_cast<uint32_t*>(S.dst + off) = *reinterpret_cast<const uint32_t*>(S.src + off);
}

__global__ __launch_bounds__(256) void snapshot_kernel(SnapTable t) {
    uint32_t k = 0;
    while (k + 1u < t.count && blockIdx.x >= t.s[k + 1u].first_block) k++;   // (uniform: scalar loads from the argument segment)
    const SnapSection& S = t.s[k];
    const uint32_t rpu = 16u / S.row_bytes;                                  // rows per unit
    const uint64_t units = (static_cast<uint64_t>(S.rows) + rpu - 1u) / rpu, whole = S.rows / rpu;
    const uint64_t u0 = static_cast<uint64_t>(blockIdx.x - S.first_block) * kSnapChunk;
    const uint64_t u1 = u0 + kSnapChunk < units ? u0 + kSnapChunk : units;
    // the chunk as a whole (uniform): every row of it moves -- no mask, or one chosen body; none does -- the workgroup has read mask
    // bytes only and leaves; or it straddles bodies of both kinds and every row asks for itself
    bool all = t.mask == nullptr;
    if (!all && S.kind == kRowsByRange) {
        const uint32_t r0 = static_cast<uint32_t>(u0 * rpu);
        const uint64_t r1x = u1 * rpu < S.rows ? u1 * rpu : S.rows;          // one past the chunk's last row
        const uint32_t b0 = body_of_row(S.table, t.bodies, r0);
        if (b0 == t.bodies) return;                                          // padding only
        const uint32_t b1 = body_of_row(S.table, t.bodies, static_cast<uint32_t>(r1x - 1u));
        if (b0 == b1) {
            if (t.mask[b0] == 0) return;
            all = true;
        } else {
            bool any = false;
            for (uint32_t b = b0; b <= b1 && b < t.bodies; b++) any |= t.mask[b] != 0;
            if (!any) return;
        }
    }
    if (all) {
        uint4 v[kSnapPerLane];
#pragma unroll
        for (uint32_t j = 0; j < kSnapPerLane; j++) {
            const uint64_t u = u0 + j * kSnapLanes + threadIdx.x;
            if (u < u1 && u < whole) v[j] = reinterpret_cast<const uint4*>(S.src)[u];
        }
#pragma unroll
        for (uint32_t j = 0; j < kSnapPerLane; j++) {
            const uint64_t u = u0 + j * kSnapLanes + threadIdx.x;
            if (u < u1 && u < whole) {
                if (S.stamped) v[j].w = 0u;
                reinterpret_cast<uint4*>(S.dst)[u] = v[j];
            } else if (u < u1) {                                             // the section's short last unit
                for (uint32_t r = static_cast<uint32_t>(u * rpu); r < S.rows; r++) move_row(S, r);
            }
        }
        return;
    }
    for (uint32_t j = 0; j < kSnapPerLane; j++) {
        const uint64_t u = u0 + j * kSnapLanes + threadIdx.x;
        if (u >= u1) break;
        const uint32_t r0 = static_cast<uint32_t>(u * rpu);
        for (uint32_t r = r0; r < r0 + rpu && r < S.rows; r++)
            if (row_chosen(S, t.mask, t.bodies, r)) move_row(S, r);
    }
}

// for which dt a prediction is valid: "any" intersected with X is X, two different dt have nothing in common (NaN: the next step predicts afresh)
void intersect_validity(bool* any_dt, float* dt, bool other_any, float other_dt) {
    if (other_any) return;
    if (*any_dt) { *any_dt = false; *dt = other_dt; return; }
    if (!(*dt == other_dt)) *dt = std::nanf("");
}

// the body tables of a masked call, uploaded once (the only blocking part of a capture or a restore, with the creation of the events)
int ensure_body_tables(tetsim_body* h) {
    if (h->d_snap_first_vert) return 0;
    std::vector<uint32_t> fv, fe;
    body_ranges(h, &fv, &fe);   // (the device's ranges too: no partitioned body gets here, so every particle and tet is local, and a body's particles keep their range)
    uint32_t* d_fe = nullptr;
    if (h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI) {
        if (int rc = dev_alloc(h, &d_fe, fe.size())) return rc;
        if (int rc = upload(h, d_fe, fe)) return rc;
        h->d_snap_first_elem = d_fe;
    } else {
        std::vector<uint32_t> body(h->nh.nt);
        for (uint32_t i = 0; i < h->nh.nt; i++) body[i] = body_of_tet(h, static_cast<uint32_t>(h->order[i]));   // volError entry i belongs to the caller's tet order[i]
        if (int rc = dev_alloc(h, &d_fe, body.size())) return rc;
        if (int rc = upload(h, d_fe, body)) return rc;
        h->d_snap_tet_body = d_fe;
    }
    uint32_t* d_fv = nullptr;
    if (int rc = dev_alloc(h, &d_fv, fv.size())) return rc;
    if (int rc = upload(h, d_fv, fv)) return rc;
    h->d_snap_first_vert = d_fv;   // (last: set only when every table is there)
    return 0;
}

// the one launch of a call on h->stream: every section, snapshot -> state (restore) or state -> snapshot
int launch_snapshot(tetsim_body* h, tetsim_snapshot_s* s, const void* mask, bool restore) {
    std::vector<StateSection> secs;
    state_sections(h, secs);
    SnapTable t{};
    t.mask = static_cast<const uint8_t*>(mask);
    t.bodies = h->info.num_bodies;
    uint32_t blocks = 0;
    auto add = [&](char* live, char* kept, uint32_t rows, uint32_t row_bytes, uint32_t kind, const uint32_t* table, bool stamped) {
        if (rows == 0 || t.count == kMaxSnapSections) return;
        SnapSection& S = t.s[t.count++];
        S.dst = restore ? live : kept; S.src = restore ? kept : live;
        S.table = table; S.rows = rows; S.row_bytes = row_bytes; S.first_block = blocks;
        S.kind = kind; S.stamped = stamped ? 1u : 0u;
        const uint64_t units = (static_cast<uint64_t>(rows) * row_bytes + 15u) / 16u;
        blocks += static_cast<uint32_t>((units + kSnapChunk - 1u) / kSnapChunk);
    };
    for (size_t i = 0; i < secs.size(); i++) {
        const StateSection& sec = secs[i];
        const bool by_table = sec.of == StateRows::kSolveOrder;
        add(static_cast<char*>(sec.ptr), static_cast<char*>(s->buf[i]), static_cast<uint32_t>(sec.rows), sec.row_bytes, by_table ? kRowsByTable : kRowsByRange,
            by_table ? h->d_snap_tet_body : sec.of == StateRows::kParticles ? h->d_snap_first_vert : h->d_snap_first_elem, sec.stamped);
    }
    if (blocks) hipLaunchKernelGGL(snapshot_kernel, dim3(blocks), dim3(kSnapLanes), 0, h->stream, t);
    return launched(h);
}

// what capture and restore refuse, before anything is enqueued (device_call_guard's two steps, with the owner's check between them as ever)
int check_call(tetsim_body* h, tetsim_snapshot_s* s, const void* mask) {
    if (!s) return fail(h, TETSIM_EINVAL, "snapshot is null");
    if (h->partitioned) return fail(h, TETSIM_ESTATE, kPartitionedIo);
    if (s->owner != h) return fail(h, TETSIM_EINVAL, "the snapshot belongs to another handle");
    HIPCHK(h, hipSetDevice(h->opt.device));
    return check_body_mask(h, mask, h->info.num_bodies);
}

void free_snapshot(tetsim_snapshot_s* s) {
    tetsim_body* h = s->owner;
    for (size_t i = 0; i < s->buf.size(); i++)
        if (s->buf[i]) { (void)hipFree(s->buf[i]); h->info.device_bytes -= s->bytes[i]; }
    delete s;
}

}  // namespace

int ensure_snapshot_body_tables(tetsim_body* h) { return ensure_body_tables(h); }   // (place.hip finds a row's body the same way)

void release_snapshots(tetsim_body* h) {   // (tetsim_destroy has drained the queues)
    for (tetsim_snapshot_s* s : h->snapshots) free_snapshot(s);
    h->snapshots.clear();
}

}  // namespace tetsim

extern "C" {

int tetsim_snapshot_create(tetsim_handle h, tetsim_snapshot* out) {
    if (!h) return TETSIM_EINVAL;
    if (!out) return fail(h, TETSIM_EINVAL, "out is null");
    *out = nullptr;
    if (int rc = device_call_guard(h)) return rc;
    std::vector<StateSection> secs;
    state_sections(h, secs);
    tetsim_snapshot_s* s = new tetsim_snapshot_s;
    s->owner = h;
    for (const StateSection& sec : secs) {
        void* p = nullptr;
        const size_t bytes = std::max<size_t>(sec.bytes(), 16);
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            free_snapshot(s);
            return fail(h, TETSIM_ENOMEM, "hipMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e));
        }
        s->buf.push_back(p);
        s->bytes.push_back(sec.bytes());
        h->info.device_bytes += sec.bytes();
    }
    int rc = ensure_quats(h);
    if (!rc) rc = launch_snapshot(h, s, nullptr, false);
    if (rc) { (void)hipStreamSynchronize(h->stream); free_snapshot(s); return rc; }
    s->pred_any_dt = h->pred_any_dt; s->dt_pred = h->dt_pred;
    h->snapshots.push_back(s);
    *out = s;
    return 0;
}

int tetsim_snapshot_capture(tetsim_handle h, tetsim_snapshot s, const void* body_mask, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (int rc = check_call(h, s, body_mask)) return rc;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (body_mask) { if (int rc = ensure_body_tables(h)) return rc; }
    return on_caller_stream(h, caller_stream, [&]() -> int {
        if (int rc = ensure_quats(h)) return rc;   // (a lean-state body: the quaternion section is what its shape section says)
        if (int rc = launch_snapshot(h, s, body_mask, false)) return rc;
        if (body_mask) intersect_validity(&s->pred_any_dt, &s->dt_pred, h->pred_any_dt, h->dt_pred);
        else { s->pred_any_dt = h->pred_any_dt; s->dt_pred = h->dt_pred; }
        return 0;
    });
}

int tetsim_snapshot_restore(tetsim_handle h, tetsim_snapshot s, const void* body_mask, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    if (int rc = check_call(h, s, body_mask)) return rc;
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (body_mask) { if (int rc = ensure_body_tables(h)) return rc; }
    return on_caller_stream(h, caller_stream, [&]() -> int {
        if (int rc = launch_snapshot(h, s, body_mask, true)) return rc;
        if (body_mask) intersect_validity(&h->pred_any_dt, &h->dt_pred, s->pred_any_dt, s->dt_pred);
        else {
            // every body comes from the snapshot: what tetsim_load_state leaves for a blob of that moment.  (After a masked restore quat_stale stays
            // as it was: pjb_recover_quat_kernel gives the same bits when it runs again on the same shape next to the quaternion it stored.)
            h->pred_any_dt = s->pred_any_dt; h->dt_pred = s->dt_pred;
            h->quat_stale = false;
        }
        return 0;
    });
}

void tetsim_snapshot_destroy(tetsim_snapshot s) {
    if (!s) return;
    tetsim_body* h = s->owner;
    (void)hipSetDevice(h->opt.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);   // (a capture or a restore may still be running)
    h->snapshots.erase(std::remove(h->snapshots.begin(), h->snapshots.end(), s), h->snapshots.end());
    free_snapshot(s);
}

}  // extern "C"
