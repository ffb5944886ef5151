// body.h -- the handle behind tetsim_handle and the helpers the translation units of the C ABI share.
//
//   tetsim_api.hip     lifecycle, stepping (streams / graphs); behind the handle below: which one-launch path serves a call (frame_now,
//                      nh_frame_now, nh_one_now) and the launchers of the handle's arithmetic mode (pj_launchers, nh_launchers)
//   tetsim_state.hip   the state's host entry points: reads (copying: on the host; pinned: through the gather), tetsim_write_state,
//                      checkpoint and resume, plan getters; state_sections(), the table of self-describing sections that IS the complete state
//   tetsim_visual.hip  embedded visual mesh (its set-up and its host reads), grab (pin, nearest-particle query), the handle's colliders; tetsim_query.hip: picking, range sensors, closest points
//   device_io.hip      how rows leave and enter the device arrays, for all of the above: the table of TETSIM_FIELD_* (source, rows, width,
//                      index map, what must run first, which requests are errors), the one gather kernel and the staging buffer of the
//                      host reads that use it; export / import in device memory; every device-side call's guard and ordering against a caller's stream
//   snapshot.hip       the complete state kept in device memory: capture and restore of chosen bodies (tetsim_snapshot_*), one copy kernel
//   body_reduce.h      what the four units below share: every body cut into chunks of 256 rows, the fixed reduction tree, the host steps
//   observe.hip        per-body observations on the device (tetsim_observe_bodies_device): mass centre, volume, tet health, bounds -- two
//                      launches over a constant per-tet table
//   strain.hip         per-tet strain on the device (tetsim_tet_strain_device / _body_strain_device / _visual_strain_device): deformation
//                      gradient, stretches, Green strain -- one lane per tet over a constant 64-byte record
//   pose.hip           per-body pose on the device (tetsim_body_poses_device): mass moments over a constant per-particle table, the best-fit
//                      rotation (Horn's quaternion by a fixed Jacobi procedure), angular velocity and momentum
//   touch.hip          touch sensing on the device (tetsim_touch_bodies_device / _particles_device): signed distance and normal of every
//                      particle against its body's colliders, per body and slot or per particle -- read-only, over the particle chunks
//   body_rows.h        what the three per-body tables below share: the one collider routine (also tetsim_set_colliders') and the one conversion
//                      of a row of parameters (also fill_params'), compiled for both sides; the host steps of a set call
//   body_grabs.hip     one held particle per body of a batch, set from host or device memory (tetsim_set_body_grabs / _device): the table the
//                      particle passes read; the nearest particle of every body on the device (tetsim_nearest_particles_device)
//   body_params.hip   physics parameters per body of a batch, set from host or device memory (tetsim_set_body_params / _device)
//   body_colliders.hip up to eight kinematic colliders per body of a batch, set from host or device memory (tetsim_set_body_colliders /
//                      _device): the table collide.h's routines walk in place of the handle's list, one set kernel, a lane per body
//   place.hip          a rigid motion of chosen bodies' complete state, rows and mask in device memory (tetsim_place_bodies / _device): one
//                      kernel over every section of state_sections(), a row's body from the snapshots' tables
//   tetsim_measure.hip measurement: per-kernel profile, kernel timing loops, device copy bandwidth
//   tetsim_create.hip  construction of the two solvers' device state (host preprocessing -> uploads)
//   tetsim_halo.hip    multi-GPU: per-substep halo choreography (two queues, flag or event synchronised), in-process group stepping
//   tetsim_comm.hip    multi-GPU set-up: RCCL communicator, self-test and probe, halo plan
//   tetsim_p2p.hip     peer-to-peer halo: export / connect (HIP IPC mappings of the neighbours' ghost ranges)
//   tetsim_host.cpp    host-only entry points: preprocessing, partition plans, the .tetsim container
//
// There is NO CPU fallback: every compute entry point needs a working HIP device and fails with
// TETSIM_ENODEVICE / TETSIM_EHIP otherwise.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/tetsim.h"
#include "dev_common.h"
#include "dev_store.h"
#include "query_device.h"
#include "host_prep.h"
#include "mesh_file.h"

namespace tetsim {

// device words of the flag-synchronised halo path (binary semaphores): [0] G, [2] V, [3] re-prediction after a dt change, [4] error, [6] [7] queue probe
constexpr uint32_t kSyncWords = 8;

// ---- RCCL, resolved at run time so single-GPU hosts (and the N-API addon) do not need librccl ----------
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
    bool loaded = false, process_wide = false;
    bool load() {
        if (loaded) return true;
        // TETSIM_RCCL_LIB: explicit library path (deployments with several RCCL builds; the test double of tests/mock_rccl)
        if (const char* over = getenv("TETSIM_RCCL_LIB")) {
            lib = dlopen(over, RTLD_NOW | RTLD_LOCAL);
            if (!lib) { err = std::string("cannot load TETSIM_RCCL_LIB=") + over + ": " + dlerror(); return false; }
        }
        // An RCCL that is ALREADY in the process (PyTorch brings its own) is the one to use: a second copy next to it is two sets of
        // the same symbols, and whichever of the two is loaded later binds some of its own calls to the other (seen on ROCm 7.2
        // boxes, where "librccl.so.1" resolves to /opt/rocm's build and PyTorch's bundled one has another name: `double free or
        // corruption` when the process exits).  So: by name without loading, then whatever the process exports, and only then a
        // fresh copy -- with LOCAL scope and DEEPBIND, so that neither copy ever resolves into the other.
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            if (lib) break;
            lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
        }
        if (!lib && dlsym(RTLD_DEFAULT, "ncclCommInitRank") && dlsym(RTLD_DEFAULT, "ncclSend")) process_wide = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            if (lib || process_wide) break;
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
        }
        if (!lib && !process_wide) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
        auto sym = [&](const char* n) { void* p = dlsym(process_wide ? RTLD_DEFAULT : lib, n); if (!p) err = std::string("librccl lacks ") + n; return p; };
        GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(sym("ncclGetUniqueId"));
        CommInitRank = reinterpret_cast<decltype(CommInitRank)>(sym("ncclCommInitRank"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
        CommCount = reinterpret_cast<decltype(CommCount)>(sym("ncclCommCount"));
        CommUserRank = reinterpret_cast<decltype(CommUserRank)>(sym("ncclCommUserRank"));
        Send = reinterpret_cast<decltype(Send)>(sym("ncclSend"));
        Recv = reinterpret_cast<decltype(Recv)>(sym("ncclRecv"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
        loaded = GetUniqueId && CommInitRank && CommDestroy && CommCount && CommUserRank && Send && Recv && GroupStart && GroupEnd && GetErrorString;
        return loaded;
    }
};
// A/B switches of choices that measurement has settled (HISTORY.md) are read by the DEVELOPMENT build only (-DTETSIM_ABLATION); the
// product library does not look at them: TETSIM_QUAD_POLL_DELAY, TETSIM_NH_QUADS, TETSIM_NH_FOLD, TETSIM_NH_FRAME, TETSIM_FRAME_LOCAL,
// TETSIM_HALO_ALIGNED_TILES.  What the product reads is what INTEGRATION.md 4 lists.
inline const char* lab_env(const char* name) {
#ifdef TETSIM_ABLATION
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}
extern Rccl g_rccl;
// Bumped whenever this library creates a stream in the process (every handle's main stream, every halo stream): HIP does not pin a
// stream to a hardware queue, so a queue-independence probe (probe_queue_independence) is only as good as the set of streams it
// was taken with -- a body re-probes before it replays its two-chain halo graphs whenever this changed since its last probe.
extern std::atomic<uint64_t> g_stream_generation;

// Peer-to-peer halo: where this rank's boundary predictions go at one neighbour -- its ghost run for this rank and the word that
// says "arrived", per substep parity -- in the neighbour's memory (an IPC mapping, a pointer of the same process, or this rank's
// own buffers in loopback measurements).
struct PeerLink {
    float4* ghost[2] = {nullptr, nullptr};
    uint32_t* arrived[2] = {nullptr, nullptr};
    void* ipc[3] = {nullptr, nullptr, nullptr};   // mappings to close (hipIpcCloseMemHandle)
    // two-layer ghost regions (TETSIM_FLAG_DEEP_GHOSTS): this rank's runs in the neighbour's four buffers, two sets each (the sets
    // alternate from one exchange to the next), and its words [set][0 = the even substep's data, 1 = the early, odd-substep data]
    float4* g1_even[2] = {nullptr, nullptr};    // predictions of the neighbour's first-layer ghosts, for its next even substep
    float4* g1_final[2] = {nullptr, nullptr};   // ... and their end-of-substep positions (the neighbour advances them itself)
    float4* g2_even[2] = {nullptr, nullptr};    // predictions of its second-layer ghosts for the even substep
    float4* g2_odd[2] = {nullptr, nullptr};     // ... and for the odd substep before it (evolves its second-layer ghost tets after the fact)
    uint32_t* arrived2[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
};
struct NeighDev {
    int rank = -1;
    uint32_t send_count = 0, recv_start = 0, recv_count = 0;
    bool contiguous = false;
    uint32_t send_first = 0;       // when contiguous: first local id
    int32_t* send_idx = nullptr;   // device, when not contiguous
    float4* send_buf = nullptr;    // device staging, when not contiguous
    std::vector<int32_t> send_global, recv_global, send_local;
};

// The per-body calls' cut of every body into chunks of 256 particles / tets (body_reduce.h: ensure_chunk_table), one table per kind,
// uploaded by the first call that needs it; `chunks` is set last
enum ChunkKind : uint32_t { kParticleChunks = 0, kTetChunks = 1 };
struct BodyChunk;
struct BodyChunks;
struct ChunkTable {
    const BodyChunk* chunks = nullptr;     // [n_chunks] {first row, rows, body}
    const BodyChunks* bodies = nullptr;    // [bodies] the body's chunks, which are also its partial rows
    uint32_t n_chunks = 0;
};

// tetsim_observe_bodies_device (observe.hip): the constant table and the scratch of a handle's observations, made by its first one
struct ObsDev {
    const void* tets = nullptr;        // [tets] int4: the four API particle ids
    const double* v0 = nullptr;        // [tets] signed rest volume
    double* partial = nullptr;         // [tet chunks + particle chunks] partial rows
    double* rows = nullptr;            // [bodies][TETSIM_OBS_WIDTH]: the device side of tetsim_read_body_observations
    bool ready = false;
};

// tetsim_tet_strain_device / tetsim_body_strain_device / tetsim_visual_strain_device (strain.hip): the constant tables and the scratch of a
// handle's strain calls, made by its first one
// The constant record of a tet (tetsim_prep_strain_table, built once on the host): 64 bytes, read by a lane as four 16-byte loads.
struct StrainRec {
    int32_t id[4];        // the four API particle ids
    float b[9];           // invRestPose, column-major, as tetsim_prep_rest returns it
    uint32_t degenerate;  // rest volume 0, or a non-finite invRestPose entry
    double v0_abs;        // |V0|, V0 the observation's
};
static_assert(sizeof(StrainRec) == 64 && alignof(StrainRec) == 8, "four dwordx4 loads per record");
struct StrainDev {
    const void* table = nullptr;       // [tets] 64-byte records: the four API particle ids, invRestPose, the degenerate mark, |V0|
    const uint32_t* vis_tet = nullptr; // [num_vis_verts] the tet of every attached visual row (the first visual call)
    double* partial = nullptr;         // [tet chunks][TETSIM_STRAIN_BODY_WIDTH] partial body rows
    float* rows = nullptr;             // [tets][TETSIM_STRAIN_WIDTH]: the device side of tetsim_read_tet_strain
    bool ready = false;
};

// tetsim_body_poses_device / tetsim_read_body_poses (pose.hip): the constant table and the scratch of a handle's pose calls, made by its
// first one.  The constant record of a particle (tetsim_prep_pose_table, built once on the host): 32 bytes, read as two 16-byte loads.
struct PoseRec {
    double m;             // lumped mass: the sum of (density * V0) / 4 over the corners that name the particle
    double q[3];          // rest position relative to the body's rest mass centre
};
static_assert(sizeof(PoseRec) == 32 && alignof(PoseRec) == 8, "two dwordx4 loads per record");
struct PoseDev {
    const void* table = nullptr;       // [particles] 32-byte records in the caller's numbering
    double* partial = nullptr;         // [particle chunks][26] chunk rows
    double* rows = nullptr;            // [bodies][TETSIM_POSE_WIDTH]: the device side of tetsim_read_body_poses
    bool ready = false;
};

// tetsim_touch_bodies_device / tetsim_read_body_touch / tetsim_touch_particles_device (touch.hip): the scratch of a handle's touch calls,
// made by its first one
struct TouchDev {
    double* partial = nullptr;         // [particle chunks][90] chunk rows
    double* rows = nullptr;            // [bodies][TETSIM_TOUCH_WIDTH]: the device side of tetsim_read_body_touch
    bool ready = false;
};

}  // namespace tetsim

using namespace tetsim;  // (private header of the ABI's own translation units; the handle type lives in the global namespace)

struct tetsim_snapshot_s;

struct tetsim_body {
    std::string err;
    TetSimOptions opt{};
    TetSimInfo info{};
    hipStream_t stream = nullptr, comm_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_bnd_tet = nullptr;
    uint32_t interior_tets = 0;         // tets of the interior tiles (blocked, partitioned)
    bool queues_probed = false, queues_independent = false;   // flag path: do the two streams run on independent hardware queues?
    uint64_t probe_generation = 0;      // g_stream_generation at the time of that probe
    std::map<uint32_t, std::pair<hipGraphExec_t, hipGraphExec_t>> flag_graphs;   // n substeps -> (main chain, halo chain), replayed side by side
    uint32_t* d_sync = nullptr;         // device counters of the flag-synchronised halo path: G done/taken, V done/taken, error
    bool flag_sync = false;             // this body steps through the flag-synchronised path (blocked + transport)
    bool halo_graph_broken = false;
    bool halo_warm = false;             // RCCL bodies: one eager call has run (connections are set up before any capture)
    bool loopback = false;              // measurement only (TETSIM_DEBUG_LOOPBACK_HALO): every neighbour is this rank itself
    bool vel_dead = false;              // the substep being enqueued is not the last of its call: its particle kernels leave the velocity array alone (nobody reads it before the call's last substep)
    bool needs_halo_refresh = false;    // in-process group: predictions were redone for a new dt
    bool fork_needed = true;            // first substep of a step call: the boundary stream must see the main stream's history
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_halo = nullptr;
    // halo choreography events, double buffered by substep parity: an event is never re-recorded while a wait that
    // other streams enqueued on its previous record may still be pending
    hipEvent_t ev_boundary2[2] = {nullptr, nullptr}, ev_packed2[2] = {nullptr, nullptr}, ev_sent2[2] = {nullptr, nullptr};
    uint32_t halo_parity = 0;
    DevParams* d_params = nullptr;
    DevParams* d_params_halo = nullptr;   // the same parameters, copied on the HALO stream (its boundary-particle pass reads them)
    std::vector<int32_t> tet_colour;  // copy of TetSimOptions.tet_colour (create only)
    int32_t grab_global = -1;
    int32_t grab_ref[2] = {-1, -1};  // particles the reference's indexFromUV pins for grab_global (TETSIM_FLAG_REF_GRAB_TEXEL)
    float grab_pos[3] = {0, 0, 0};
    // kinematic colliders (tetsim_set_colliders), normalised, in the two views fill_params copies into DevParams
    uint32_t n_colliders = 0;
    DevColliderF col[kMaxColliders] = {};
    DevColliderD d_col[kMaxColliders] = {};
    // body grabs (tetsim_set_body_grabs / _device, body_grabs.hip): one held particle per body.  The table -- the body of every particle in
    // device order, a 16-byte row per body -- is made by the first set call and keeps its addresses (fill_params copies them into
    // DevParams); ON / OFF is host state and travels as DevParams::body_grabs.  Not solver state: no checkpoint or snapshot holds it.
    bool body_grabs_on = false;
    uint32_t* d_grab_body = nullptr;    // [particles]; made by whichever of body grabs and body colliders is set first (ensure_particle_bodies)
    int4* d_grab_rows = nullptr;        // [bodies]
    // body pins (tetsim_set_body_pins / _device, body_pins.hip): any number of held particles per body.  Per particle in device order the
    // row that holds it (-1 = free) and pin_per_body rows of the same 16 bytes per body; the slots are made by the first set call and keep
    // their address, the rows are made anew when per_body changes.  ON / OFF is host state and travels as DevParams::body_grabs ==
    // kHoldBodyPins, with the rows' address in DevParams::grab_rows.  Not solver state either.
    bool body_pins_on = false;
    int32_t* d_pin_slot = nullptr;      // [particles]
    int4* d_pin_rows = nullptr;         // [bodies * pin_per_body]
    size_t pin_rows_cap = 0;
    uint32_t pin_per_body = 0;
    // body colliders (tetsim_set_body_colliders / _device, body_colliders.hip): per body a count and kMaxColliders compacted entries, in the
    // view this handle's arithmetic reads (f32: polar, FAST Neo-Hookean; f64: PRECISE Neo-Hookean -- the other pointer stays null).  Made by
    // the first set call, every body empty; ON / OFF is host state and travels as DevParams::body_colliders.  Not solver state either.
    bool body_colliders_on = false;
    uint32_t* d_bcol_count = nullptr;   // [bodies]
    DevColliderF* d_bcol_f = nullptr;   // [bodies][kMaxColliders]
    DevColliderD* d_bcol_d = nullptr;   // [bodies][kMaxColliders]
    // body parameters (tetsim_set_body_params / _device, body_params.hip): a row per body -- gravity, friction, the two compliances, the bounds --
    // in the view this handle's arithmetic reads (the other pointer stays null), and for Neo-Hookean handles the body of every tet in the
    // device's tet order.  Made by the first set call, every body at tetsim_default_params(); ON / OFF is host state and travels as
    // DevParams::body_params.  Not solver state either.
    bool body_params_on = false;
    BodyParamsF* d_bp_f = nullptr;      // [bodies]
    BodyParamsD* d_bp_d = nullptr;      // [bodies]
    uint32_t* d_tet_body = nullptr;     // [tets] Neo-Hookean only
    uint32_t* d_body_first = nullptr;   // [bodies + 1] first particle of every body in the CALLER's numbering (also tetsim_nearest_particles_device)
    // tetsim_nearest_particles_device: a candidate per chunk of the particle chunk table (below)
    double* d_near_d2 = nullptr;
    uint32_t* d_near_id = nullptr;
    std::map<uint32_t, hipGraphExec_t> graphs;
    std::vector<void*> allocs;
    std::vector<float> h_verts;
    std::vector<int32_t> h_tets;
    // tetsim_create_batch: first particle / first tet of every body in the concatenation, [bodies + 1]; empty = a single body
    std::vector<uint32_t> batch_first_vert, batch_first_tet;
    bool fast = false;

    // POLAR_JACOBI
    PJDev pj;
    PJBlk blk;             // blocked formulation (FAST unless TETSIM_FLAG_GATHER_FORMULATION)
    bool blocked = false;
    // fused particle pass (unpartitioned blocked bodies): tetsim_step_n runs  tet | fused x (n-1) | particle  instead of n x (tet | particle)
    bool halo_use_flags = true;       // TETSIM_HALO_SYNC (read when the body is created): false = "events", the older event-synchronised halo path
    bool halo_use_graph = true;       // TETSIM_HALO_GRAPH (likewise): false = the halo path stays eager
    bool fused = false;
    // large unpartitioned blocked bodies (two kernels per substep): tetsim_step_n runs a CALL as ONE launch -- per substep the tiles, then the
    // particles, handed on by stamped partial sums and predictions (pj_blocked.hip: pjb_call_kernel); TETSIM_PJ_ONE_LAUNCH=0 at creation keeps
    // two kernels per substep (A/B); tetsim_step and tetsim_profile keep the two kernels (same arithmetic, same bits)
    bool pj_one_launch = false;
    uint32_t* d_substep_err = nullptr;
    // ... in the order of a host-built dispatch table (host_prep.h: CallSchedule; TETSIM_PJ_CALL_LAG at creation, 0 = every tile, then every particle block)
    PJCallSched call_sched;
    // TETSIM_FLAG_LEAN_STATE (pj_blocked.hip: kModeLeanState): the substep neither reads nor writes pj.quat; it is recovered from the carried
    // shape and this constant centred rest shape when somebody asks for it (ensure_quats)
    float4 *rest0_a = nullptr, *rest0_b = nullptr, *rest0_c = nullptr;
    bool quat_stale = false;          // substeps have been enqueued since pj.quat was last recovered
    // persistent frame kernel (pjb_frame_kernel): tetsim_step_n runs ONE launch per call; fused bodies of few enough tiles
    bool frame = false;               // (whether it serves the call at hand: frame_now, behind this struct)
    uint32_t frame_epoch = 1;         // sequence number of the next call's first substep (DevParams::epoch), advanced by 65536 per parameter push
    uint32_t fold_wave_limit = 0, fold_tile_limit = 0;   // waves / workgroups that may wait in-kernel on this device (pjb_wait_capacity, at creation)
    bool quad = false;                // SMALL body: 64-tet tiles, one tet / one particle on four lanes (pj_quad.hip) -- tetsim_step runs pjq_tet + pjq_vertex,
                                      // tetsim_step_n the persistent pjq_frame_kernel (while `frame`); the three agree bit for bit
    uint32_t* d_frame_err = nullptr;  // raised by a tile whose neighbour's partial sums never arrived (bounded wait)
    int32_t* d_block_tile = nullptr;  // [frame_blocks] tile of every block of the frame kernel's grid, -1 = none
    uint32_t frame_blocks = 0;
    DevParams params_on_device;       // what d_params holds (valid while params_known)
    bool params_known = false;
    bool frame_local = false;         // every body's tiles share one XCD: the exchange is coherent in that XCD's L2 (pjb_frame_kernel_local)
    bool frame_turn_counted = false;  // this body is in its device's count of exclusive bodies
    bool epoch_block_fresh = false;   // push_params took a block of sequence numbers that no launch has used yet
    bool frame_exclusive = false;     // needs MORE than half the device's resident workgroups: persistent launches of this device take turns (tetsim_api.hip: FrameTurn)
    float4* partial_b = nullptr;      // second buffer of the tile partial sums
    size_t partial_slots = 0;         // float4s in each of the two
    float4* pos_final_b = nullptr;    // second buffer of the end-of-substep positions (a call always ENDS in pj.pos_final)
    bool fold_halo = false;           // peer-to-peer halo: the halo-side tiles do their queue's hand-overs themselves (TETSIM_HALO_FOLD_WAIT=0: a wait kernel in front)
    bool fold_possible = false;       // ... this body could (interior tiles and interior particles exist, not switched off)
    bool fold_wait = false;           // flag path: the interior particle kernel awaits G itself (TETSIM_HALO_FOLD_WAIT=0 at creation: a wait kernel in front of it)
    bool v_pending = false;           // flag path: the interior particles of the last enqueued substep are not signalled yet (flush_v)
    uint32_t fuse_step = 0;           // substep index inside the current run (enqueue_substep)
    bool fin_in_b = false;            // the latest end-of-substep positions are in pos_final_b (only between the kernels of one call)
    std::vector<int32_t> tet_perm;  // blocked: device tet position -> local tet index
    // Particles are renumbered on the device (Morton order inside the interior segment) for locality; the API keeps
    // the caller's / the partition plan's numbering.  api2dev[a] = device index of API-local particle a.
    std::vector<uint32_t> api2dev, dev2api;
    Partition part;
    bool partitioned = false;
    std::vector<int32_t> g2l_owned;  // global vertex -> local id (owned) or -1
    std::vector<NeighDev> neigh;
    bool pred_any_dt = true;  // velocities are all zero: the prediction is valid for every dt
    float dt_pred = 0.0f;
    ncclComm_t comm = nullptr;
    int comm_rank = -1, comm_size = 0;
    // peer-to-peer halo (tetsim_halo_p2p_export / _connect): no transfer kernel -- the boundary-particle kernel stores into the
    // neighbours' ghost ranges, double buffered by substep parity (pos_pred's tail | ghost_alt)
    // two-layer ghost region (TETSIM_FLAG_DEEP_GHOSTS): ghosts [nv_owned, nv_owned + n_ghost1) are advanced here on even substeps,
    // the second-layer ghost tets are tiles [nb_first, nb) -- solved on even substeps, evolved after the fact on odd ones
    bool deep = false;
    uint32_t n_ghost1 = 0, nb_first = 0;
    std::vector<int32_t> g2l_ghost1;      // global vertex -> local id of a first-layer ghost, or -1 (grab)
    bool p2p = false;
    uint32_t timeout_ms = 0;              // bound of the device-side waits of this body (TETSIM_HALO_TIMEOUT_MS when it was created / connected)
    float4* ghost_alt = nullptr;          // [nv_local - nv_owned] the ghost buffer of odd substeps
    uint32_t* d_arrived = nullptr;        // [2][kMaxPeers] words the neighbours raise here
    uint32_t* d_peer_slots = nullptr;     // ELL [p2p_cols][p2p_stride]: where a boundary particle goes at which neighbour
    uint32_t p2p_cols = 0, p2p_stride = 0;
    uint32_t* d_peer_slots2 = nullptr;    // two-layer regions: the same for the neighbours' SECOND layer (disjoint lists)
    uint32_t p2p_cols2 = 0;
    // two-layer regions, own receive buffers: ghost_alt holds [g1_even x2 | g1_final x2 | g2_even x2 | g2_odd x2]
    float4* own_g1_even[2] = {nullptr, nullptr};
    float4* own_g1_final[2] = {nullptr, nullptr};
    float4* own_g2_even[2] = {nullptr, nullptr};
    float4* own_g2_odd[2] = {nullptr, nullptr};
    std::vector<PeerLink> links;          // parallel to `neigh`
    uint32_t p2p_probe_base = 0;          // tetsim_halo_p2p_probe: the inbox words count on from here (every rank calls it the same number of times)
    uint64_t p2p_round = 0;               // substeps enqueued since the connection; its parity selects the buffers
    bool p2p_raise_pending = false;       // the last boundary-particle kernel's "arrived" has not been raised yet (no kernel behind it)
    bool halo_pending = false;            // a halo was started and nobody has waited for it yet
    bool final_ghosts_fresh = false;      // pos_final's ghost range holds the neighbours' END-OF-SUBSTEP positions of the current state (tetsim_halo_refresh_final)
    std::vector<tetsim_body*> group;      // in-process group transport: partition i of the decomposition (or empty)

    SkinDev skin;  // embedded visual mesh
    std::vector<uint32_t> vis_tet;     // the tet (caller's numbering) that carries each attached visual vertex
    std::vector<int32_t> vis_global;   // row of the caller's visVerts behind each attached visual vertex (a partition keeps the rows of the tets it owns)
    bool vis_attached = false;
    uint32_t vis_total = 0;            // rows of the caller's visVerts (a partition keeps num_vis_verts of them)
    float4* d_vis_full = nullptr;      // partitions with visual triangles: every rank's skin put together, [vis_total] (tetsim_visual_vertex_normals_from)
    float* pinned_pos = nullptr;   // tetsim_read_positions_pinned: host-pinned xyz
    float* d_packed = nullptr;     // staging of the pinned and the visual reads: packed rows, grown to the largest request so far (read_rows)
    size_t packed_cap = 0;         //   floats in it
    float* pinned_quat = nullptr;  // tetsim_read_quats_pinned: host-pinned xyzw per local tet
    uint32_t* d_api2dev = nullptr; // device copy of api2dev (gather / scatter / nearest kernels), null = identity
    // tetsim_export_device / tetsim_import_device (device_io.hip): [call parity][0 = recorded on the caller's stream, 1 = on h->stream],
    // created by the first such call; double buffered like the halo events above
    hipEvent_t ev_io[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    uint32_t io_parity = 0;
    // tetsim_snapshot_* (snapshot.hip): the snapshots this handle still owns; the body of every row, uploaded by the first masked call --
    // [bodies + 1] first particle / first tet in device numbering, and for a Neo-Hookean batch the body of every volError entry
    std::vector<tetsim_snapshot_s*> snapshots;
    uint32_t *d_snap_first_vert = nullptr, *d_snap_first_elem = nullptr, *d_snap_tet_body = nullptr;
    // tetsim_place_bodies (place.hip): where the host variant's rows and mask wait for the kernel, made by its first call
    float* d_place_rows = nullptr;      // [bodies][TETSIM_PLACE_WIDTH]
    uint8_t* d_place_mask = nullptr;    // [bodies]
    ChunkTable chunk_table[2];     // [ChunkKind]: what the per-body calls reduce over (body_reduce.h)
    ObsDev obs;                    // tetsim_observe_bodies_device / tetsim_read_body_observations (observe.hip)
    StrainDev strain;              // tetsim_tet_strain_device / tetsim_body_strain_device / tetsim_visual_strain_device (strain.hip)
    PoseDev pose;                  // tetsim_body_poses_device / tetsim_read_body_poses (pose.hip)
    TouchDev touch;                // tetsim_touch_bodies_device / tetsim_read_body_touch / tetsim_touch_particles_device (touch.hip)
    double* d_best = nullptr; uint32_t* d_best_id = nullptr;  // tetsim_start_grab candidates
    // tetsim_raycast_visual / tetsim_read_visual_bounding_sphere (query_kernels.hip): allocated by the first query, grown on demand
    uint32_t* d_sphere = nullptr;
    RayIn* d_rays = nullptr; RayPrep* d_ray_prep = nullptr; RayOut* d_ray_hits = nullptr; RayCand* d_ray_cand = nullptr;
    size_t ray_cap = 0, ray_prep_cap = 0, ray_hits_cap = 0, ray_cand_cap = 0;   // elements in d_rays / d_ray_prep / d_ray_hits / d_ray_cand
    std::vector<int32_t> vis_row_body, tri_body;   // batches: the body behind every visual row / behind every triangle's first vertex
    // tetsim_raycast_visual_device / tetsim_visual_bounding_spheres_device (query_device.h): the per-body tables of the visual mesh, uploaded
    // by the first such call (rows: either call; triangles: the ray call), and the candidates of the few-ray launches
    QueryBodiesDev qbodies;
    bool qrows_ready = false, qtris_ready = false;
    bool tri_spans_bodies = false;     // some triangle's three rows belong to different bodies: no per-body cast
    RayCand* d_cast_cand = nullptr;    // [kCastCandCap]
    // tetsim_raycast_visual_bvh_device (query_bvh.hip): the tree over every body's triangles, its topology built by the first such call
    BvhDev bvh;
    bool bvh_ready = false;
    // tetsim_closest_visual (query_closest.hip): where the host variant's queries, bodies and records wait, grown on demand
    PointQueryIn* d_point_queries = nullptr; int32_t* d_point_bodies = nullptr; ClosestOut* d_closest = nullptr;
    size_t point_query_cap = 0, point_body_cap = 0, closest_cap = 0;

    // NEOHOOKEAN_GS
    NHDev nh;
    std::vector<NHClusterLaunch> cluster_launch;  // TETSIM_ORDER_CLUSTERED: one per cluster colour
    int32_t* d_slot_vid = nullptr;
    // clustered schedule: the particle pass between two substeps of a run is folded into the sweep's first touchers
    // (NHClusterLaunch::first_mask); nh_untouched lists the particles no cluster touches, which keep a (tiny) pass of their own
    bool nh_fold = false;
    uint8_t* d_first_mask = nullptr;
    uint32_t* d_nh_untouched = nullptr;
    uint32_t nh_untouched = 0;
    // clustered FAST bodies: the sweep as ONE launch per substep, particles handed on with their stamp (dev_common.h: NHSweep);
    // TETSIM_NH_ONE_LAUNCH=0 at creation keeps one launch per colour (A/B); tetsim_profile always does (it times the colour kernels)
    bool nh_one_launch = false;       // (whether it serves the call at hand: nh_one_now, behind this struct)
    bool nh_call = false;             // ... and tetsim_step_n runs the sweeps of ALL its substeps as one launch (nh_call_kernel: every particle touched by some cluster, <= 127 colours)
    NHSweep nh_sweep1;
    uint32_t nh_sub_index = 0;        // substep inside the run being enqueued (enqueue_substep: first -> 0)
    uint32_t nh_epoch_arg = 0;        // tetsim_step: a block of stamps of its own as a kernel argument; 0 = DevParams::epoch (tetsim_step_n)
    std::vector<uint32_t> level_off;
    // small bodies (all particles fit one CU's LDS, level schedules): tetsim_step_n runs a call as ONE single-workgroup launch
    bool nh_frame = false;            // (whether it serves the call at hand: nh_frame_now, behind this struct)
    NHFrameLaunch nh_frame_launch;
    std::vector<uint32_t> nh_seg;      // host copy of nh_frame_launch.seg ([levels][bodies][2]): the stepwise FAST twin makes the frame kernel's choice per piece
    std::vector<int32_t> order;
    std::vector<float> h_inv_mass;
};

namespace tetsim {

// ---- whether a one-launch flag of the handle (frame, nh_frame, nh_one_launch above) serves the call at hand: the flag says what the body
// was built for, a per-body switch may take it off that path for as long as it is on.  Every stepping decision asks these, never the pair.
// The persistent frame kernel serves this call -- not while a quad body has body colliders on: pjq_frame_kernel has no register for a second
// kind of list (pj_quad.hip: pjq_vertex_update), the body then takes the two launches per substep that tetsim_profile and the fall-back
// take, which agree with the frame kernel bit for bit.
// Nor while a body of the 256-tet tiles has body pins on: pjb_frame_kernel is compiled without them (with them it lost a wave of occupancy:
// dev_common.h, body_grab_pick), the body then steps through the fused kernels, which agree with the frame kernel bit for bit.
inline bool frame_now(const tetsim_body* h) { return h->frame && !(h->quad && h->body_colliders_on) && !(!h->quad && h->body_pins_on); }
// Likewise the Neo-Hookean calls that are one launch: nh_frame_kernel, nh_sweep1_kernel and nh_call_kernel keep the parent's particle pass
// (with the second list they lose a wave of occupancy or gain a stack: nh_kernels.inc, post_vertex), so while body colliders are on the
// body steps through the level / cluster kernels and the particle kernels, which take the table and agree with them bit for bit.
inline bool nh_frame_now(const tetsim_body* h) { return h->nh_frame && !h->body_colliders_on; }
inline bool nh_one_now(const tetsim_body* h) { return h->nh_one_launch && !h->body_colliders_on; }
// ---- the launchers of the handle's arithmetic mode (dev_common.h: one table per solver, an instance per mode)
inline const PJLaunchers& pj_launchers(const tetsim_body* h) { return h->fast ? pj_launchers_fast : pj_launchers_precise; }
inline const NHLaunchers& nh_launchers(const tetsim_body* h) { return h->fast ? nh_launchers_fast : nh_launchers_precise; }

// ---- the bodies of a handle (here alone: batch_first_* are empty for a single body).  is_batch: made by tetsim_create_batch, of however many bodies
inline bool is_batch(const tetsim_body* h) { return !h->batch_first_vert.empty(); }
// [bodies + 1] first particle / first tet of every body in the caller's (API) numbering, for a batch and for a single body alike
inline void body_ranges(const tetsim_body* h, std::vector<uint32_t>* first_vert, std::vector<uint32_t>* first_tet) {
    *first_vert = h->batch_first_vert; *first_tet = h->batch_first_tet;
    if (!is_batch(h)) { *first_vert = {0u, h->info.num_particles}; *first_tet = {0u, h->info.num_elems}; }
}
inline uint32_t body_of_tet(const tetsim_body* h, uint32_t t) {   // t: a tet in the caller's numbering
    const std::vector<uint32_t>& first = h->batch_first_tet;
    return first.empty() ? 0u : static_cast<uint32_t>(std::upper_bound(first.begin(), first.end(), t) - first.begin()) - 1u;
}

// V0 of a tet as the observations and the strain rows define it: dot(r1-r0, cross(r2-r0, r3-r0)) / 6 of the f32 rest positions in f64,
// with its sign (observe.hip: obs_volume is the same expression on the device); for units built with -ffp-contract=off
inline double rest_volume(const float* v, const int32_t* t) {
    const float *a = v + 3 * t[0], *b = v + 3 * t[1], *c = v + 3 * t[2], *d = v + 3 * t[3];
    const double e1x = static_cast<double>(b[0]) - a[0], e1y = static_cast<double>(b[1]) - a[1], e1z = static_cast<double>(b[2]) - a[2];
    const double e2x = static_cast<double>(c[0]) - a[0], e2y = static_cast<double>(c[1]) - a[1], e2z = static_cast<double>(c[2]) - a[2];
    const double e3x = static_cast<double>(d[0]) - a[0], e3y = static_cast<double>(d[1]) - a[1], e3z = static_cast<double>(d[2]) - a[2];
    const double cx = e2y * e3z - e2z * e3y, cy = e2z * e3x - e2x * e3z, cz = e2x * e3y - e2y * e3x;
    return ((e1x * cx + e1y * cy) + e1z * cz) / 6.0;
}

// a float a device row may hold (place.hip, body_grabs.hip): neither infinite nor NaN, by its bits
__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

void build_strain_table(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, double density, StrainRec* out);   // tetsim_host.cpp
// first_vert: [bodies + 1] first particle of every body; centres: [3 * bodies] the bodies' rest mass centres, or null
void build_pose_table(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, const uint32_t* first_vert, uint32_t bodies, double density,
                      PoseRec* out, double* centres);   // tetsim_host.cpp

#define HIPCHK(h, call)                                                                                 \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                               \
            return TETSIM_EHIP;                                                                         \
        }                                                                                               \
    } while (0)

int fail(tetsim_body* h, int code, const std::string& msg);  // records the message on the handle (or for tetsim_last_error(NULL))
const char* create_error();
void group_begin(tetsim_body* const* hs, uint32_t count);             // entry points over several handles: clear the members' messages ...
int group_result(tetsim_body* const* hs, uint32_t count, int rc);     // ... and publish the failing member's for tetsim_last_error(NULL)

template <class Tp>
inline int dev_alloc(tetsim_body* h, Tp** p, size_t count) {
    *p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(Tp);
    void* raw = nullptr;
    hipError_t e = hipMalloc(&raw, bytes);
    if (e != hipSuccess) { h->err = std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e); return TETSIM_ENOMEM; }
    h->allocs.push_back(raw);
    h->info.device_bytes += bytes;
    *p = static_cast<Tp*>(raw);
    return 0;
}
// a buffer that grows on demand: the old one is released (and leaves device_bytes) before the larger one is allocated
template <class Tp>
inline int dev_grow(tetsim_body* h, Tp** p, size_t* cap, size_t need) {
    if (*p && need <= *cap) return 0;
    if (*p) {
        h->allocs.erase(std::find(h->allocs.begin(), h->allocs.end(), static_cast<void*>(*p)));
        (void)hipFree(*p);
        h->info.device_bytes -= std::max<size_t>(*cap, 1) * sizeof(Tp);
        *p = nullptr;
    }
    *cap = 0;
    const int rc = dev_alloc(h, p, need);
    if (rc == 0) *cap = need;
    return rc;
}
template <class Tp>
inline int upload(tetsim_body* h, Tp* dst, const std::vector<Tp>& src) {
    if (src.empty()) return 0;
    HIPCHK(h, hipMemcpy(dst, src.data(), src.size() * sizeof(Tp), hipMemcpyHostToDevice));
    return 0;
}

// SoftbodyGPU.js:335-338,345: texel (px,py) of the R x R position texture is pinned when

void ref_grab_texels(int32_t grab_id, uint32_t num_elems, uint32_t num_particles, int32_t out[2]);
// reuse_ok: the caller's kernels do not need a fresh block of sequence numbers (tetsim_step) -- if the parameters equal what the device
// already holds, nothing is uploaded
int push_params(tetsim_body* h, double dt, const TetSimParams* params, bool reuse_ok = false);

// Development: TETSIM_DEBUG_HOSTPROF=1 accumulates the host time of every call in the eager halo path, printed at destroy.
struct HostProf {
    bool on = [] { const char* e = getenv("TETSIM_DEBUG_HOSTPROF"); return e && e[0] == '1'; }();
    std::map<std::string, std::pair<double, uint64_t>> acc;
    ~HostProf() { for (auto& kv : acc) fprintf(stderr, "[hostprof] %-28s %8.2f us avg over %llu calls\n", kv.first.c_str(), kv.second.first / kv.second.second, (unsigned long long)kv.second.second); }
};
extern HostProf g_hostprof;
struct HostProfScope {
    const char* label; std::chrono::steady_clock::time_point t0;
    explicit HostProfScope(const char* l) : label(l) { if (g_hostprof.on) t0 = std::chrono::steady_clock::now(); }
    ~HostProfScope() { if (g_hostprof.on) { auto& a = g_hostprof.acc[label]; a.first += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); a.second++; } }
};
#define HP(label) HostProfScope hp_scope_##__LINE__(label)

// ---- kernel sequencing (tetsim_api.hip)
void pj_tet(tetsim_body* h, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
void pj_vertex(tetsim_body* h, uint32_t first, uint32_t count, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
void pj_fused_substep(tetsim_body* h, bool first, bool last, hipEvent_t* e);   // one substep of a fused body (tet | fused x (n-1) | particle)
void pj_repredict(tetsim_body* h);
void nh_sweep(tetsim_body* h, bool fold = false, bool last = true, bool one_launch = false);   // one_launch: bodies with nh_one_launch take the single-launch sweep (enqueue_substep; tetsim_profile keeps the colour kernels)   // fold: first touchers do the particle pass between two substeps; last: the sweep whose volError the call leaves behind
// first / last: position inside a run of substeps enqueued back to back with one dt
int enqueue_substep(tetsim_body* h, bool first = true, bool last = true);
int ensure_prediction(tetsim_body* h, double dt);
// ---- state read-back helpers (tetsim_state.hip)
const float4* current_positions(tetsim_body* h);   // end-of-substep positions of either solver
int ensure_quats(tetsim_body* h);                  // lean-state bodies: pj.quat brought up to date on h->stream (behind both queues' work); else nothing
int ensure_index_map(tetsim_body* h);              // device copy of api2dev (gather / scatter / nearest kernels)
// What the complete solver state is: the device arrays a checkpoint holds one after the other, and a snapshot one buffer each.  A
// section says what it is, so that no reader needs the handle to interpret it; a new state array is added in state_sections() alone.
enum class StateRows : uint8_t {
    kParticles,    // particles in device numbering (a body's particles keep their range)
    kTets,         // tets in the device's own order: blocked tile order, or caller order on the gather path (elem: one section per plane, the rows behind nt are nobody's)
    kSolveOrder,   // tets by position in the Neo-Hookean solve sequence (vol_err[order[e]]): a coloured or clustered order interleaves the bodies
};
struct StateSection {
    void* ptr;
    size_t rows; uint32_t row_bytes;   // 16, 8 or 4
    StateRows of;         // whose rows they are
    bool stamped;         // the fourth float of a 16-byte row is a call's sequence number and leaves as 0 (tetsim_api.hip: next_epoch_block)
    bool predictions;     // polar pos_pred: a peer-to-peer body on odd substep parity keeps its ghost tail in ghost_alt
    size_t bytes() const { return rows * row_bytes; }
};
void state_sections(tetsim_body* h, std::vector<StateSection>& v);
// ---- rows out of and into the device arrays (device_io.hip)
int drain(tetsim_body* h);                         // set the device, wait for h->stream, then for h->comm_stream if there is one
struct FieldSrc {                                  // a TETSIM_FIELD_* on this body: row r = `width` floats of src[mapped ? d_api2dev[r] : r]
    const float4* src = nullptr;
    uint32_t rows = 0, width = 3;
    bool mapped = false;
    bool quats = false, skin = false, vnrm = false;   // what runs first: quaternion recovery, skinning, vertex normals
};
// 0, or TETSIM_ESTATE / TETSIM_EINVAL and in *why the reason the body has no such field (host_reader: in the tetsim_read_* wording)
int resolve_field(tetsim_body* h, int32_t field, bool host_reader, FieldSrc* f, std::string* why);
int prepare_fields(tetsim_body* h, const FieldSrc* f, uint32_t count);   // once per request, on h->stream: index map, quaternions, skin, vertex normals
// the pinned reads and the visual mesh's reads: comm_stream drained, prepare_fields, then read_rows -- the gather into the staging buffer on h->stream and one copy per
// field to out[k], behind a stream sync (pinned: an async copy in stream order, then the sync); count <= TETSIM_MAX_EXPORT_FIELDS
int read_fields(tetsim_body* h, const FieldSrc* f, float* const* out, uint32_t count, bool pinned = false);
// (on its own for tetsim_visual_vertex_normals_from, which computes the normals of the caller's positions and must not skin first)
int read_rows(tetsim_body* h, const FieldSrc* f, float* const* out, uint32_t count, bool pinned = false);
// the stream contract of the device-side calls: the two events of this call, the first recorded on the caller's stream and awaited by
// the handle's (io_begin); the second recorded on the handle's stream and awaited by the caller's (io_end)
int io_begin(tetsim_body* h, hipStream_t caller, hipEvent_t** ev);
int io_end(tetsim_body* h, hipStream_t caller, hipEvent_t* ev);
// ... and a call under that contract, behind its argument checks: io_begin, what `enqueue` puts on h->stream (non-zero ends the call), io_end
template <class F> int on_caller_stream(tetsim_body* h, void* caller_stream, F&& enqueue) {
    hipStream_t const cs = static_cast<hipStream_t>(caller_stream);
    hipEvent_t* ev;
    if (int rc = io_begin(h, cs, &ev)) return rc;
    if (int rc = enqueue()) return rc;
    return io_end(h, cs, ev);
}
int device_call_guard(tetsim_body* h);             // what every device-side call starts from: not a partitioned body (kPartitionedIo), the handle's device set
int launched(tetsim_body* h);                      // hipGetLastError behind a kernel launch
// `ptr` is device memory of the handle's device and `need` bytes from it fit the allocation it points into (`misfit`: the message if not)
int check_device_span(tetsim_body* h, const void* ptr, uint64_t need, const std::string& what, const std::string& misfit);
// records of `row_bytes` in the caller's device memory: a stride is 0 (packed) or a multiple of `align` of at least the record; `ptr` is not
// null, aligned to `align`, device memory of the handle's device, and `rows` records `stride` bytes apart (the resolved stride) fit its allocation
bool record_stride_ok(uint64_t stride, uint64_t row_bytes, uint32_t align);
int check_device_records(tetsim_body* h, const void* ptr, uint64_t stride, uint32_t rows, uint64_t row_bytes, uint32_t align, const std::string& what);
extern const char* const kPartitionedIo;           // the refusal of a partitioned body, one text for every device-side call
extern const char* const kBodyGrabsOn;             // the refusal of the handle's grab while body grabs are on (body_grabs.hip)
extern const char* const kBodyPinsOn;              // the refusal of the handle's grab and of body grabs while body pins are on (body_pins.hip)
extern const char* const kBodyCollidersOn;         // the refusal of a non-empty handle list while body colliders are on (body_colliders.hip)
// what the per-body tables start from (body_grabs.hip; the first call of each may block)
uint32_t num_bodies(const tetsim_body* h);
int ensure_body_first(tetsim_body* h);             // d_body_first and the index map
int ensure_particle_bodies(tetsim_body* h);        // d_grab_body: the body of every particle in DEVICE particle order
void release_snapshots(tetsim_body* h);            // tetsim_destroy: the snapshots that are left (snapshot.hip)
int ensure_snapshot_body_tables(tetsim_body* h);   // d_snap_first_vert / _first_elem / _tet_body, uploaded once (snapshot.hip: ensure_body_tables; may block)

// ---- construction (tetsim_create.hip)
int create_polar(tetsim_body* h, const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt);
int create_neohookean(tetsim_body* h, const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt);

// ---- halo (tetsim_halo.hip)
int create_halo_stream(tetsim_body* h);
int rccl_fail(tetsim_body* h, ncclResult_t r, const char* what);
int halo_start(tetsim_body* h);
int halo_wait(tetsim_body* h, hipStream_t on);
uint32_t halo_timeout_ms(const tetsim_body* h = nullptr);   // the body's bound, or the environment's
bool has_transport(const tetsim_body* h);
bool uses_flag_sync(const tetsim_body* h);
int enqueue_phase_a(tetsim_body* h, hipEvent_t* ev = nullptr);  // tet kernels + particles; ev[0..3]: begin/end of the interior tet and the particle kernel
int flush_v(tetsim_body* h);                                    // flag path: the V hand-over that no following substep will carry
int enqueue_phase_b(tetsim_body* h, bool refresh = false);      // halo start (peer-to-peer bodies: only for the refresh after a dt change)
float4* ghost_buffer(tetsim_body* h, uint32_t parity);          // where ghost particle nv_owned + i of that substep parity lives (+ i)
int probe_queue_independence(tetsim_body* h);                   // flag path: may the two chains be replayed from graphs?
int step_n_flag_graphs(tetsim_body* h, uint32_t n);             // n substeps of an RCCL flag-path body as two captured chains
void frame_turn_enter(tetsim_body* h);                         // an exclusive persistent-launch body joins its device's turn-taking (tetsim_api.hip)
int refresh_final_rccl(tetsim_body* h);                         // RCCL bodies: the ghosts' end-of-substep positions into pos_final's ghost range (collective)
void drop_flag_graphs(tetsim_body* h);                          // destroy the captured chains (queues turned out not to be independent)

}  // namespace tetsim
