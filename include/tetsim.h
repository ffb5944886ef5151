/*
 * tetsim.h -- C ABI of libtetsim_hip.so: the MI355X-native XPBD tetrahedral soft-body hot path.
 *
 * This is the drop-in boundary for the per-substep solve of zalo/TetSim.  Every entry point replaces
 * one piece of the reference's `SoftBody` / `SoftBodyGPU` surface (citations are file:line under the
 * reference tree); the N-API shim (tetsim_amd/node/tetsim_napi.cc) and the ctypes host
 * (tetsim_amd/softbody.py) bind these 1:1.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a TETSIM_E* code; tetsim_last_error() gives the text
 *     (the reference reports init problems as an error *string*, SoftbodyGPU.js:379-380);
 *   - all inputs are copied at create; device memory is owned by the handle;
 *   - step calls enqueue work on the handle's HIP stream and return WITHOUT synchronising;
 *     reads synchronise;
 *   - a handle is not thread-safe (the reference is single-threaded JS, World.js:73).
 *   - numbers that are JS `number`s in the reference (dt, physicsParams) are doubles here so the
 *     Neo-Hookean path can reproduce Softbody.js's f64-arithmetic/f32-store results bit for bit.
 */
#ifndef TETSIM_H
#define TETSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TETSIM_ABI_VERSION 5

typedef struct tetsim_body *tetsim_handle;

/* error codes */
enum {
    TETSIM_OK = 0,
    TETSIM_EINVAL = 1,    /* bad argument (null pointer, index out of range, repeated vertex in a tet ...) */
    TETSIM_ENODEVICE = 2, /* no usable HIP device / HIP extension not functional: never falls back to CPU */
    TETSIM_EHIP = 3,      /* a HIP runtime call failed; text in tetsim_last_error */
    TETSIM_ENOMEM = 4,
    TETSIM_ECOMM = 5,     /* RCCL load/init/transfer failure */
    TETSIM_ESTATE = 6     /* call not valid for this handle (e.g. quats of a Neo-Hookean body) */
};

/* which of the reference's two solvers */
enum {
    TETSIM_SOLVER_POLAR_JACOBI = 0,  /* SoftbodyGPU.js: shape-matching / polar decomposition, Jacobi (7 GLSL passes :59-376) */
    TETSIM_SOLVER_NEOHOOKEAN_GS = 1  /* Softbody.js:  Neo-Hookean XPBD, Gauss-Seidel (:91-240) */
};

/* arithmetic mode */
enum {
    /* POLAR_JACOBI: IEEE f32, no FMA contraction, correctly rounded div/sqrt, libm-grade sin -- op-for-op the
     *               GLSL source order.  NEOHOOKEAN_GS: f64 arithmetic with f32 stores exactly where
     *               Softbody.js rounds (bit-exact with the reference CPU solver). */
    TETSIM_PRECISE = 0,
    /* f32 throughout, FMA contraction, hardware rcp/rsq/sin.  Tolerance-level parity (tests state it). */
    TETSIM_FAST = 1
};

/* Gauss-Seidel element order (NEOHOOKEAN_GS only) */
enum {
    /* exactly the sequential order of the caller's tetIds (Softbody.js:207-208), parallelised by
     * dependency levels: two tets run concurrently only if no earlier/later pair shares a vertex. */
    TETSIM_ORDER_ORIGINAL = 0,
    /* greedy graph colouring, tets stably sorted by colour (BASELINE config 4).  The result equals the
     * reference CPU solver run on tetIds permuted by tetsim_get_tet_order(). */
    TETSIM_ORDER_COLOURED = 1,
    /* clusters of <= 8 tets over <= 8 vertices (the 6 tets of a cell on a cell-major lattice), clusters coloured; a GPU lane
     * sweeps its cluster sequentially out of LDS, one launch per cluster colour (8 on the lattice instead of 31 tet colours).
     * Same contract as COLOURED: the result equals the reference CPU solver run on tetIds permuted by
     * tetsim_get_tet_order().  TetSimInfo.num_levels = launches per substep; tet_colour is ignored. */
    TETSIM_ORDER_CLUSTERED = 2
};

/* flags */
enum {
    /* build the particle->(tet,vertex) scatter table exactly as SoftbodyGPU.js:563-577 does, including
     * its `<= 0.0` empty-slot test (:568), which drops tet 0 / vertex 0's contribution, and the 36-slot
     * cap.  Without it every incident tet contributes. */
    TETSIM_FLAG_REF_SLOT_TABLE = 1u << 0,
    /* ignore params.worldBounds and clamp to the constants hard-coded in the collision pass
     * (SoftbodyGPU.js:347).  POLAR_JACOBI only; on by default through tetsim_default_options(). */
    TETSIM_FLAG_REF_FIXED_BOUNDS = 1u << 1,
    /* POLAR_JACOBI + FAST normally runs the blocked formulation (workgroup tiles, LDS-staged particles,
     * per-tile partial sums).  This flag keeps the gather formulation (reference slot order). */
    TETSIM_FLAG_GATHER_FORMULATION = 1u << 2,
    /* POLAR_JACOBI + FAST + blocked: do not carry the rotated rest shape in world space (48 B/tet read + 48 B/tet written
     * per substep, as the reference's textureElem does) but re-derive it as R(q) * rest0 from the quaternion and a constant
     * centred rest shape (SURVEY.md 8(a) design note): identical in exact arithmetic, ~30% less tet-kernel traffic;
     * rounding differs (tolerance-level).  Measured +4% tet-solves/s (the tet kernel is issue-bound).  Off by default: the benchmark measures the reference formulation. */
    TETSIM_FLAG_CONSTANT_REST_SHAPE = 1u << 3,
    /* POLAR_JACOBI: pin the particle(s) the reference's collision pass actually pins.  Its indexFromUV
     * (SoftbodyGPU.js:335-338, "This isn't quite correct") maps texel (px,py) of the R x R position texture to
     * int(uv.x*(R-1)) + int(uv.y*(R-1)*R), not to px + R*py, so `grabId` selects zero, one or two OTHER particles.
     * Off by default (the library pins exactly grabId); on for bit-faithful replays of the reference's grab. */
    TETSIM_FLAG_REF_GRAB_TEXEL = 1u << 4,
    /* partitioned POLAR_JACOBI + TETSIM_FAST (blocked): a ghost region TWO layers deep.  The partition advances its first ghost layer
     * itself and its neighbours' particles cross only every other substep -- half the hand-overs on the substep's critical chain
     * (DESIGN.md 7).  Needs the peer-to-peer halo (tetsim_halo_p2p_connect) before the first step; dt must stay fixed. */
    TETSIM_FLAG_DEEP_GHOSTS = 1u << 5,
    /* POLAR_JACOBI + TETSIM_FAST: end a tet's rotation iterations only where the reference does (|omega| < 1e-9,
     * SoftbodyGPU.js:131 -- unreachable in f32 unless the tet is exactly rigid, so all nine run).  Without the flag FAST ends the
     * CORRECTION iterations 2..9 of a tet (of a wavefront, when all its tets agree) once |omega| < 1e-6 rad: an order of magnitude
     * below the rotation that f32 position rounding alone induces in a centimetre-sized tet a metre from the origin (iteration 1 of
     * a rigid free fall reads 1e-6..3e-5, profiles/r04_rotation_iterations.txt).  Iteration 1 always keeps the reference's test.
     * PRECISE ignores this flag: it always is the reference. */
    TETSIM_FLAG_REF_ROTATION_EXIT = 1u << 6,
    /* POLAR_JACOBI + FAST + blocked: the LEAN tet record (since ABI 5).  The reference streams per tet and substep the carried
     * ("last rotated") rest shape in and out (SoftbodyGPU.js:253-262: 4 corners, 48 B each way) and its quaternion in and out
     * (:181, 16 B each way): 148 B with the staged positions and the weight.  Two of those items are redundant in FAST arithmetic:
     * (a) the quaternion is PURE OUTPUT of a substep -- the rotation applied to the shape is this substep's `rel` alone -- and the
     * carried shape IS the accumulated rotation applied to the rest shape, so the quaternion is recovered from the shape when it
     * is asked for (tetsim_read_quats, the visual mesh, tetsim_save_state) instead of being multiplied up every substep;
     * (b) the shape is kept relative to its own centroid, so its fourth corner is minus the sum of the other three.
     * 92 B per tet instead of 148.  Rounding differs from the default FAST path at tolerance level (the fourth corner is rebuilt,
     * not carried; the read-out quaternion is R = C S0^-1 -> q, equal to the multiplied-up one to ~1e-6, and equal in SIGN as long as
     * a tet turns by less than pi between two read-outs); a zero-volume tet reads back the quaternion it was created with.  Small
     * bodies take the 256-tet-tile kernels (TetSimInfo.fused_particle_pass 2, not 3).  Excludes _CONSTANT_REST_SHAPE and _DEEP_GHOSTS.
     * Off by default: the benchmark's headline measures the reference's formulation, `value_lean` this one (bench.py). */
    TETSIM_FLAG_LEAN_STATE = 1u << 7
};

/* physicsParams (main.js:22-36) -- the keys the hot path reads each substep. */
typedef struct TetSimParams {
    double gravity;        /* Softbody.js:199 ; SoftbodyGPU.js:371 */
    double friction;       /* Softbody.js:224-225 ; SoftbodyGPU.js:352 */
    double devCompliance;  /* Softbody.js:130,161 (NEOHOOKEAN_GS) */
    double volCompliance;  /* Softbody.js:161,165 (NEOHOOKEAN_GS) */
    double worldBounds[6]; /* lo xyz, hi xyz ; Softbody.js:215-216 */
} TetSimParams;

typedef struct TetSimOptions {
    int32_t solver;     /* TETSIM_SOLVER_* */
    int32_t precision;  /* TETSIM_PRECISE / TETSIM_FAST */
    int32_t order;      /* TETSIM_ORDER_* (NEOHOOKEAN_GS) */
    uint32_t flags;     /* TETSIM_FLAG_* */
    int32_t device;     /* HIP device ordinal */
    double density;     /* physicsParams.density, consumed at construction (Softbody.js:32,74) */
    /* Domain decomposition (POLAR_JACOBI).  part_count <= 1: whole mesh on this handle.  Otherwise this
     * handle owns the vertices v with vert_owner[v] == part_index (vert_owner == NULL: the built-in
     * partitioner, tetsim_prep_partition without coordinates) plus a ghost layer; see DESIGN.md 7. */
    int32_t part_count;
    int32_t part_index;
    const int32_t *vert_owner;
    /* NEOHOOKEAN_GS + TETSIM_ORDER_COLOURED: a caller-supplied colour per tet, [num_elems], or NULL for the built-in greedy
     * colouring.  ANY labelling is safe: the solve order is "stable sort by colour", and the parallel levels are derived
     * from that order's true dependencies, so a poor colouring costs speed, never correctness (since ABI 2). */
    const int32_t *tet_colour;
} TetSimOptions;

typedef struct TetSimInfo {
    uint32_t num_particles;      /* vertices of the caller's (global) mesh  -- SoftBody.numParticles */
    uint32_t num_elems;          /* tets of the caller's (global) mesh      -- SoftBody.numElems */
    uint32_t owned_particles;    /* vertices this handle integrates (== num_particles when unpartitioned) */
    uint32_t local_particles;    /* owned + ghost */
    uint32_t local_elems;        /* tets this handle solves (owned + ghost tets) */
    uint32_t owned_elems;        /* tets counted once across partitions (lowest-owner rule) */
    uint32_t num_levels;         /* Gauss-Seidel dependency levels / colours (0 for POLAR_JACOBI) */
    uint32_t max_valence;        /* max incident tets per vertex used by the scatter table */
    uint32_t dropped_slots;      /* (tet,vertex) contributions dropped by TETSIM_FLAG_REF_SLOT_TABLE */
    uint32_t num_neighbours;     /* partitions this handle exchanges a halo with */
    uint64_t device_bytes;       /* HBM allocated by this handle so far: buffers of the read-out and query calls are allocated by the first
                                    call that needs them (the staging buffer of the pinned reads, tetsim_read_visual_mesh and
                                    tetsim_read_visual_vertex_normals by the first of those, grown to the largest request) and count from then on */
    int32_t solver, precision, order, device;
    uint32_t flags;
    uint32_t num_vis_verts;      /* visual vertices attached by tetsim_set_visual_mesh / a .tetsim file (0 = none); since ABI 3 */
    uint32_t num_bodies;         /* independent bodies behind this handle (tetsim_create_batch), 1 otherwise; since ABI 3 */
    uint32_t fused_particle_pass; /* 1: tetsim_step_n runs ONE kernel per substep (particle update fused into the tet kernel's staging,
                                     HISTORY.md 5.4: unpartitioned POLAR_JACOBI + FAST blocked bodies); tetsim_profile then times that kernel.
                                     2: ... and the body is small enough for tetsim_step_n to run ONE persistent kernel per CALL (every
                                     tile's workgroup resident for all n substeps); tetsim_profile still
                                     uses the per-substep kernels, whose results are the same bit for bit.
                                     3: as 2, on 64-tet tiles with one tet and one particle on FOUR lanes (pj_quad.hip: the default for
                                     small carried-rest-shape bodies); tetsim_profile runs the same substep as two launches.  (2 and 3:
                                     tetsim_step is the persistent kernel for ONE substep -- one launch per call.)
                                     4: NEOHOOKEAN_GS, level schedules (TETSIM_ORDER_ORIGINAL / _COLOURED), at most 4,096 particles (PRECISE: and 12,288 tets): they all
                                     fit one CU's LDS and tetsim_step_n -- and tetsim_step -- run a whole call as ONE launch of one workgroup (one per body of a batch)
                                     (nh_kernels.inc); tetsim_profile keeps one launch per level, same arithmetic, same results bit for bit
                                     5: (since ABI 5) POLAR_JACOBI + FAST blocked bodies that keep a tet and a particle kernel per substep (0: >= 2,048 tiles, or a
                                     particle no tile sums): tetsim_step_n runs a whole CALL as ONE launch -- per substep the tiles' workgroups, then the particles',
                                     substep after substep in one grid, partial sums and predictions handed on with the substep's sequence number in their fourth
                                     float (pj_blocked.hip: pjb_call_kernel); tetsim_step and tetsim_profile keep the two kernels, same results bit for bit
                                     (0 remains: partitioned bodies, PRECISE / gather bodies, TETSIM_PJ_ONE_LAUNCH=0) */
    uint32_t total_vis_verts;    /* rows of the visVerts the caller attached (num_vis_verts of them are this handle's: all, unless partitioned); since ABI 5 */
} TetSimInfo;

/* per-kernel HIP-event timing of eagerly launched substeps (tetsim_profile) */
enum { TETSIM_K_TET = 0, TETSIM_K_VERTEX = 1, TETSIM_K_HALO = 2, TETSIM_K_COUNT = 3 };
typedef struct TetSimProfile {
    double total_ms;                 /* wall on the stream for all substeps */
    double kernel_ms[TETSIM_K_COUNT]; /* summed duration per kernel class */
    uint32_t launches[TETSIM_K_COUNT];
    uint32_t substeps;
    uint32_t tets_per_tet_launch;    /* tets one timed TETSIM_K_TET launch processes: all of them, or on a partitioned body with a
                                        halo transport the INTERIOR tiles' (the halo-side tiles -- those touching a ghost or a boundary particle --
                                        run beside them on the halo stream, as do the boundary particles: TETSIM_K_VERTEX then times the
                                        interior particles' kernel) */
} TetSimProfile;

/* --- lifecycle ------------------------------------------------------------------------------- */

/* Fill `o` with the defaults that mirror the reference's GPU demo path
 * (POLAR_JACOBI, PRECISE, REF_SLOT_TABLE|REF_FIXED_BOUNDS, density 1000, device 0, unpartitioned). */
void tetsim_default_options(TetSimOptions *o);
/* physicsParams defaults of main.js:22-36. */
void tetsim_default_params(TetSimParams *p);

/* Replaces `new SoftBody(vertices, tetIds, ...)` (Softbody.js:4-58 + initPhysics :60-87) and
 * `new SoftBodyGPU(...)` (SoftbodyGPU.js:5-56 + initPhysics :487-608): copies the mesh, builds rest
 * data / tables on the host, uploads.  verts = [3*nv] xyz, tets = [4*nt] vertex ids. */
int tetsim_create(const float *verts, uint32_t nv, const int32_t *tets, uint32_t nt,
                  const TetSimOptions *opts, tetsim_handle *out);
/* Several INDEPENDENT bodies behind one handle (the reference steps `softBodies[]` one after the other, main.js:80-84): body b is
 * (verts[b], nv[b], tets[b], nt[b]); the handle's particles / tets are their concatenation (tetsim_get_batch_layout gives the
 * ranges) and every other entry point works on that concatenation -- one tetsim_step_n steps all bodies with ONE launch per
 * kernel: a Dragon-sized body alone fills 15 of the chip's 2,048 workgroup slots, sixty-four of them 960.  All bodies share
 * physicsParams (unless tetsim_set_body_params gives each its own); tetsim_set_grab addresses a particle of the concatenation.  Each body's results equal its solo run BIT FOR BIT
 * (both solvers, both precisions): tiles never span two bodies and are cut per body exactly as for a body alone, the
 * reference's slot-table quirk applies to every body's own first tet, Gauss-Seidel schedules of disjoint bodies are independent
 * (tetsim_get_tet_order then refers to the concatenation).  Unpartitioned only. */
int tetsim_create_batch(const float *const *verts, const uint32_t *nv, const int32_t *const *tets, const uint32_t *nt,
                        uint32_t count, const TetSimOptions *opts, tetsim_handle *out);
/* first_particle / first_elem [num_bodies + 1]: body b owns particles [first_particle[b], first_particle[b+1]) of the handle. */
int tetsim_get_batch_layout(tetsim_handle h, uint32_t *first_particle, uint32_t *first_elem);
void tetsim_destroy(tetsim_handle h);

/* Text of the last error on this handle.  h == NULL: the last error, on this thread, of a failed create or of an entry point that takes
 * SEVERAL handles (tetsim_group_step_n, tetsim_group_refresh_final, tetsim_halo_exchange_local: "partition <i>: <text>"). */
const char *tetsim_last_error(tetsim_handle h);
int tetsim_get_info(tetsim_handle h, TetSimInfo *info);

/* --- the hot path ---------------------------------------------------------------------------- */

/* Replaces `simulate(dt, physicsParams)` (Softbody.js:195-240 ; SoftbodyGPU.js:610-641): ONE substep,
 * enqueued on the handle's stream, no synchronisation. */
int tetsim_step(tetsim_handle h, double dt, const TetSimParams *params);
/* n substeps with the same dt/params/grab as one host call and one launch: the body of the caller's substep loop (main.js:79-84).
 * One replay of a captured HIP graph -- or, where the whole call is ONE kernel (TetSimInfo.fused_particle_pass 5: large
 * unpartitioned POLAR_JACOBI FAST bodies), that kernel launched directly with the call's parameters among its arguments. */
int tetsim_step_n(tetsim_handle h, uint32_t n, double dt, const TetSimParams *params);
/* Block until everything enqueued on the handle's stream(s) has finished.  Partitioned bodies: TETSIM_ECOMM if a device-side
 * halo wait gave up (TETSIM_HALO_TIMEOUT_MS, 30 s by default: a stuck peer, or the two chains of a graph replay sharing one
 * hardware queue).  The substeps since then used stale data: go back to the last checkpoint -- every rank loads the blob it saved
 * with tetsim_save_state at the same substep count (partitions save and load their own, since ABI 4), or rebuilds its partition
 * (same owner map), loads it there and re-attaches the transport -- and the trajectory continues bit for bit.  The handle itself
 * stays usable and steps eagerly (no graph replay of the halo chains) from then on. */
int tetsim_sync(tetsim_handle h);

/* --- state access (synchronising) ------------------------------------------------------------ */

/* Replaces reading `.pos` (Softbody.js:12) / readToCPU (SoftbodyGPU.js:649-653): xyz of the OWNED
 * particles after the last completed substep, [3*owned_particles], in tetsim_get_owned_ids order. */
int tetsim_read_positions(tetsim_handle h, float *out);
/* Zero-copy variant: positions are packed to xyz on the device and copied straight into a pinned
 * host buffer owned by the handle ([3*owned_particles] floats, valid until tetsim_destroy, overwritten by the next
 * call).  *out receives its address: a host wraps it once (N-API external ArrayBuffer, numpy view) and every
 * endFrame() is one device pack kernel + one DMA, no intermediate host copy.  Synchronises. */
int tetsim_read_positions_pinned(tetsim_handle h, const float **out);
int tetsim_read_prev_positions(tetsim_handle h, float *out); /* .prevPos */
int tetsim_read_velocities(tetsim_handle h, float *out);     /* .vel */
/* POLAR_JACOBI: per-tet rotation quaternion xyzw (textureQuat, SoftbodyGPU.js:55,181), [4*local_elems]
 * in tetsim_get_local_tets order. */
int tetsim_read_quats(tetsim_handle h, float *out);
/* Zero-copy variant of tetsim_read_quats (SURVEY.md §8(f)-2 "position/quaternion"; the normal path of SoftbodyGPU.js:440
 * consumes textureQuat every frame): one DMA straight into a pinned host buffer owned by the handle ([4*local_elems]
 * floats in tetsim_get_local_tets order, valid until tetsim_destroy, overwritten by the next call).  Synchronises. */
int tetsim_read_quats_pinned(tetsim_handle h, const float **out);
/* NEOHOOKEAN_GS: `.volError` of the last substep (Softbody.js:163,206,209), summed in the caller's
 * tet order in f64. */
int tetsim_read_vol_error(tetsim_handle h, double *out);
/* Overwrite positions and velocities of the owned particles.  NEOHOOKEAN_GS: that is the whole solver state.
 * POLAR_JACOBI also carries per-tet state (quaternions and the rotated rest shape, SoftbodyGPU.js:49-55 `elems`/`quats`),
 * which this call leaves untouched: to continue a trajectory use tetsim_save_state / tetsim_load_state. */
int tetsim_write_state(tetsim_handle h, const float *pos, const float *vel);
/* Checkpoint / resume of the COMPLETE solver state (both solvers): positions, velocities and, for POLAR_JACOBI, every tet's
 * quaternion and carried rest shape -- everything the reference keeps in its ping-pong render targets (SoftbodyGPU.js:49-55).
 * The blob is only meaningful for a body created from the same mesh with the same options by the same library build family (it
 * starts with a header that tetsim_load_state validates: magic, ABI, solver, precision, flags, counts, and a digest of the mesh --
 * vertices, tets, density, batch layout -- so that a blob of ANOTHER mesh with the same counts is rejected too).  A body restored
 * from a blob continues the original trajectory bit for bit.  Both calls synchronise (both streams; for the partitions of an
 * in-process group the streams of every member: a neighbour's transfer lands in this body's ghost range).
 * PARTITIONED bodies (since ABI 4): every partition saves and loads ITS OWN blob -- its owned particles, its ghosts (the predictions
 * its neighbours sent for the next substep are state too) and its local tets incl. ghost tets; the digest also covers the cut
 * (part_count, part_index, the owner map as this partition sees it), so a blob of another decomposition is rejected.  All ranks save
 * at the same substep count (after tetsim_sync) and restore together: a multi-GPU run that lost a rank rebuilds its partitions with
 * the same owner map, loads the last set of blobs, re-attaches the transport and continues bit for bit.  Transport state is not in
 * the blob (semaphore words are at rest after a sync; the peer-to-peer halo's substep parity stays the restored body's own).
 * ONE RANK PER PROCESS with the peer-to-peer halo (since ABI 5): a neighbour stores into this rank's ghost range from ITS queues, which
 * this rank cannot drain.  tetsim_save_state therefore waits (bounded: TETSIM_HALO_TIMEOUT_MS, TETSIM_ECOMM) until every neighbour's
 * predictions of the last substep have arrived, and never writes into a receive buffer -- a rank may save while its neighbours are
 * already stepping on; no barrier is needed around a save beyond "every rank saves after the same number of substeps".
 * tetsim_load_state overwrites both ghost buffers: the CALLER brackets the ranks' loads with barriers -- no rank loads before every
 * rank has synchronised (tetsim_sync), no rank steps before every rank has loaded (tests/test_gpu_p2p_halo.py shows the sequence).
 * TETSIM_FLAG_LEAN_STATE bodies: the blob holds three carried corners per tet and the quaternions as recovered at the save.  Not
 * supported: bodies with a two-layer ghost region (TETSIM_FLAG_DEEP_GHOSTS). */
int tetsim_state_size(tetsim_handle h, uint64_t *bytes_out);
int tetsim_save_state(tetsim_handle h, void *blob, uint64_t bytes);
int tetsim_load_state(tetsim_handle h, const void *blob, uint64_t bytes);

/* global vertex id of each owned particle, [owned_particles] (identity when unpartitioned) */
int tetsim_get_owned_ids(tetsim_handle h, int32_t *out);
/* global tet id of each local tet, [local_elems] */
int tetsim_get_local_tets(tetsim_handle h, int32_t *out);
/* NEOHOOKEAN_GS: the order in which tets are solved, as indices into the caller's tetIds, [num_elems]. */
int tetsim_get_tet_order(tetsim_handle h, int32_t *out);
/* NEOHOOKEAN_GS: first solve-order position of every level, [num_levels + 1]. */
int tetsim_get_level_offsets(tetsim_handle h, int32_t *out);
/* rest data as the reference computes it (Softbody.js:60-87): invMass [nv] */
int tetsim_read_inv_mass(tetsim_handle h, float *out);

/* --- embedded visual mesh --------------------------------------------------------- */

/* Attach the embedded visual mesh: vis_verts = [4*nvis] rows (tetNr, b0, b1, b2) exactly as the reference's
 * `visVerts` (Dragon.js:1705; Softbody.js:46,263-267).  rest_normals = [3*nvis] object-space normals or NULL.
 * PARTITIONED bodies (since ABI 4) take the same, global list on every rank and keep the rows whose tet they OWN (lowest-owner rule,
 * TetSimInfo.owned_elems: exactly one partition per tet, and that partition solves the tet); TetSimInfo.num_vis_verts is the number
 * kept, tetsim_get_visual_ids their row numbers -- the union over the partitions is the whole visual mesh, each row once. */
int tetsim_set_visual_mesh(tetsim_handle h, const float *vis_verts, uint32_t nvis, const float *rest_normals);
/* row of the caller's vis_verts behind each attached visual vertex, [num_vis_verts] ascending (identity when unpartitioned) */
int tetsim_get_visual_ids(tetsim_handle h, int32_t *out);
/* Skin on the device and read back.  positions_out [3*num_vis_verts]: sum_k b_k * pos[tet corner k] with b3 = 1-b0-b1-b2,
 * evaluated like updateVisMesh (Softbody.js:259-277: f64 accumulate, f32 store per step; NEOHOOKEAN_GS + PRECISE is
 * bit-exact with it) or like the vertex shader of SoftbodyGPU.js:429-435 (POLAR_JACOBI, f32).
 * normals_out [3*num_vis_verts] (may be NULL): Rotate(rest_normal, quat[tetNr]) as SoftbodyGPU.js:440 -- POLAR_JACOBI only.
 * A PARTITION returns its own rows (tetsim_get_visual_ids order); scattered by row number, the partitions' outputs equal the
 * unpartitioned body's bit for bit (PRECISE).  Corners it does not own need their owner's END-OF-SUBSTEP position, which the
 * per-substep halo does not carry (it carries predictions): every rank calls tetsim_halo_refresh_final (RCCL; in-process groups:
 * tetsim_group_refresh_final) after the frame's last substep, THEN reads.  The read itself never communicates (since ABI 5; before,
 * RCCL bodies ran the exchange from inside it, and ranks that disagreed on whether it was due hung each other): with stale ghosts
 * it fails with TETSIM_ESTATE.  A freshly created partition is fresh (its ghost range holds the rest positions). */
int tetsim_read_visual_mesh(tetsim_handle h, float *positions_out, float *normals_out);
/* The end-of-substep positions of this partition's ghost particles, from their owners, into the ghost range behind
 * tetsim_read_positions' owned range (what tetsim_read_visual_mesh needs; valid until the next step).  RCCL bodies: a collective of
 * all ranks (one grouped send / recv per neighbour on the main stream, after a sync).  Unpartitioned: nothing to do. */
int tetsim_halo_refresh_final(tetsim_handle h);
/* The same for the partitions of an in-process group (device copies). */
int tetsim_group_refresh_final(tetsim_handle *handles, uint32_t count);
/* The visual mesh's triangle list, as the reference hands it to the geometry index (Dragon.js `dragonAttachedTriIds`;
 * Softbody.js:48-50, SoftbodyGPU.js:455-457): [3*ntri] ids of visual vertices.  Needed by tetsim_read_visual_vertex_normals. */
int tetsim_set_visual_triangles(tetsim_handle h, const int32_t *tri_ids, uint32_t ntri);
/* `visMesh.geometry.computeVertexNormals()` (Softbody.js:273, every frame -- 37 ms of the CPU path's frame, SURVEY.md §8(f)-1;
 * SoftbodyGPU.js:687 when physicsParams.computeNormals) on the device, for the positions tetsim_read_visual_mesh returns:
 * three.js r160 BufferGeometry.computeVertexNormals (indexed) + normalizeNormals -- face normal (pC-pB) x (pA-pB) in f64 from
 * the f32 positions, added to the triangle's three vertices in triangle order with an f32 store per add, then scaled by
 * 1/(length || 1) in f64 and stored f32.  Each vertex gathers its triangles in that order, so the result equals the
 * reference's bit for bit (golden recorded from three.js).  normals_out [3*nvis].  Synchronises. */
int tetsim_read_visual_vertex_normals(tetsim_handle h, float *normals_out);
/* PARTITIONED bodies (since ABI 5): tetsim_set_visual_triangles takes the same, GLOBAL triangle list on every rank (ids = rows of the
 * caller's visVerts) and keeps, for each row the partition skins, that row's triangles in triangle order.  A triangle's corners may be
 * skinned by different ranks, so the normals are computed from the ranks' skins put together: the host scatters every rank's
 * tetsim_read_visual_mesh rows by tetsim_get_visual_ids into one [3 * rows of visVerts] array (it needs that array to draw anyway) and
 * every rank calls tetsim_visual_vertex_normals_from with it -> normals_out [3*num_vis_verts], this rank's rows.  Per vertex the same
 * face normals are added in the same order as in the unpartitioned body: scattered by row, the ranks' normals equal
 * tetsim_read_visual_vertex_normals of the unpartitioned body bit for bit (Softbody.js:259-277).  tetsim_read_visual_vertex_normals
 * itself refuses partitions.  An unpartitioned body may call it too (normals of any positions of its visual mesh). */
int tetsim_visual_vertex_normals_from(tetsim_handle h, const float *all_positions, float *normals_out);
/* The partitions of one process, all at once: every member skins its rows (after tetsim_group_refresh_final), the rows are put
 * together, every member computes its rows' normals from the whole.  positions_out / normals_out [3 * rows of visVerts]; either may be
 * NULL. */
int tetsim_group_read_visual_vertex_normals(tetsim_handle *handles, uint32_t count, float *positions_out, float *normals_out);

/* --- grab (Softbody.js:279-298 ; SoftbodyGPU.js:692-712) --------------------------------------- */

/* Pin global particle `id` (-1 = none, endGrab) at xyz: consumed by the next substeps
 * (Softbody.js:233-235 ; SoftbodyGPU.js:345, with the exact particle index -- see DESIGN.md). */
int tetsim_set_grab(tetsim_handle h, int32_t id, const float xyz[3]);
/* startGrab: nearest particle to xyz among the latest positions -- argmin on the device (f64 distances evaluated as
 * Softbody.js:284-288 does, first minimum wins), only one candidate per 256 particles travels to the host; sets and
 * returns the particle (no full read-back, unlike GPUGrabber.start, SoftbodyGPU.js:790-795). */
int tetsim_start_grab(tetsim_handle h, const float xyz[3], int32_t *id_out);
/* The owned particle nearest to xyz (same f64 distance and first-minimum rule) WITHOUT grabbing it: global id and squared
 * distance.  Partitioned bodies: take the minimum over the partitions on the host (ties: lowest id), then call
 * tetsim_set_grab(id, xyz) on every partition -- only the owner pins it. */
int tetsim_nearest_particle(tetsim_handle h, const float xyz[3], int32_t *global_id, double *dist2);

/* --- picking: ray casts and the bounding sphere of the visual mesh ----------------------------- */

/* Grabber.start / GPUGrabber.start (Softbody.js:440-456, SoftbodyGPU.js:788-811) cast the pointer's ray against visMesh with
 * three.js's Raycaster -- the reference's GPU path reads the mesh back for it (:789-795) -- and every endFrame ends with
 * geometry.computeBoundingSphere() (Softbody.js:256,276; SoftbodyGPU.js:689).  Both run here on the device, on the positions the
 * skinning kernel produces.  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct changed).
 *
 * tetsim_raycast_visual: for every ray the FIRST entry of what three.js r160
 *     new Raycaster(origin, direction, near, far).intersectObject(visMesh)
 * returns for a THREE.Mesh with an identity world matrix, a front-side material and an indexed BufferGeometry whose `position`
 * holds what tetsim_read_visual_mesh returns and whose index is the list given to tetsim_set_visual_triangles -- bit for bit:
 * hit (0/1), distance, point, triangle (three's faceIndex: the triangle's position in the caller's list) and body (the body of a
 * batch whose tets carry the triangle's first vertex; 0 for a single body).  A miss: hit 0, body -1, triangle -1, zeros.
 * The definition (three's Mesh.raycast, checkGeometryIntersection, Ray.intersectTriangle, restated; tests/raycast_ref.py is the
 * same in numpy, pinned to three's own answers): f64 arithmetic on the f32 positions, every operation rounded separately, sums
 * left to right, dot(u, v) = u.x*v.x + u.y*v.y + u.z*v.z.
 *   1. The bounding-sphere cull, with (centre, radius) of tetsim_read_visual_bounding_sphere and the direction as given:
 *      o2 = origin + direction*near; unless |o2 - centre|^2 <= radius^2:  v = centre - o2, tca = v.direction,
 *      d2 = v.v - tca*tca; a miss if d2 > radius^2; thc = sqrt(radius^2 - d2), t0 = tca - thc, t1 = tca + thc; a miss if t1 < 0;
 *      at = o2 + direction*(t0 < 0 ? t1 : t0); a miss if |o2 - at|^2 > (far - near)^2.
 *   2. The ray in the mesh's local space: the origin as given; the direction goes through Vector3.transformDirection, which
 *      NORMALISES it: dir = direction * (1 / (sqrt(direction.direction) || 1)).  (A unit vector computed in f64 may change in its
 *      last bits; distances are lengths in world units whatever the given direction's length.)
 *   3. Per triangle (a, b, c): e1 = b - a, e2 = c - a, n = e1 x e2, DdN = dir.n; DdN > 0 is a back face and is culled, DdN == 0
 *      misses; sign = -1, DdN = -DdN; diff = origin - a; DdQxE2 = sign * dir.(diff x e2) >= 0; DdE1xQ = sign * dir.(e1 x diff) >= 0;
 *      DdQxE2 + DdE1xQ <= DdN; QdN = -sign * diff.n >= 0; point = origin + dir*(QdN / DdN); distance = |origin - point| (the
 *      square root of the sum of squares); kept iff near <= distance <= far.
 *   4. The winner is the smallest distance, the LOWEST triangle index among equal distances (three sorts with a stable sort).
 * TETSIM_EINVAL: a null pointer with count > 0; a non-finite origin or direction; a zero direction; near < 0; far < near; a NaN
 * in near or far (far may be +infinity).  TETSIM_ESTATE: no visual mesh or no triangles attached; a partitioned body (a
 * triangle's corners may be skinned by different ranks, as for tetsim_read_visual_vertex_normals).  count == 0 succeeds; any
 * count works (the launches are chunked by the grid limits).  The call skins first, like tetsim_read_visual_mesh, so the answer
 * belongs to the last completed substep; it synchronises once and changes no solver state.
 * Out of scope: partitioned bodies; all hits along a ray; back-side or double-side materials; the edge wireframe's LineSegments;
 * an acceleration structure behind THIS call (brute force: every ray against every triangle; the per-body device casts have one:
 * tetsim_raycast_visual_bvh_device); closest-point queries (tetsim_closest_visual_device, below, answers them). */
typedef struct TetSimRay    { double origin[3], direction[3], near, far; } TetSimRay;       /* far may be +inf */
typedef struct TetSimRayHit { int32_t hit, body, triangle, reserved; double distance, point[3]; } TetSimRayHit;
int tetsim_raycast_visual(tetsim_handle h, const TetSimRay *rays, uint32_t count, TetSimRayHit *hits);
/* Grabber.start in one call: cast `ray`; on a hit the point origin + direction*distance (f64, Softbody.js:449-450) rounded to f32
 * goes through exactly what tetsim_start_grab does (*id_out = the grabbed particle); on a miss the grab stays as it was,
 * *id_out = -1 and the call returns TETSIM_OK.  hit_out and id_out may be NULL.  Unpartitioned bodies only.  The grabbed point uses
 * the direction AS GIVEN times the world-length distance, as Grabber.start does: for a direction that is not a unit vector it is not
 * hit_out->point (setFromCamera hands over a unit vector). */
int tetsim_start_grab_ray(tetsim_handle h, const TetSimRay *ray, TetSimRayHit *hit_out, int32_t *id_out);
/* three.js r160 BufferGeometry.computeBoundingSphere() of the positions tetsim_read_visual_mesh returns, bit for bit: centre =
 * (min + max) * 0.5 of the component-wise f64 min / max, radius = sqrt(max_i |centre - p_i|^2), the difference taken as
 * centre - p.  TETSIM_ESTATE: no visual mesh, or a partitioned body. */
int tetsim_read_visual_bounding_sphere(tetsim_handle h, double centre[3], double *radius);

/* --- kinematic colliders ------------------------------------------------------------------------ */

/* Obstacles the body cannot enter: spheres, capsules, oriented boxes and half-spaces, moved by the host between calls.  An
 * ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look the symbol up.
 *
 * The list is handle state, like the grab: it takes effect at the next step call and stays fixed for every substep of that call.
 * One list applies to every body of a batch; each partition takes the list its caller gives it and applies it to every particle it
 * advances (first-layer ghosts of TETSIM_FLAG_DEEP_GHOSTS included).  It is not solver state: tetsim_save_state blobs do not hold it.
 *
 * Per particle and substep the colliders run AFTER the reference's clamp, floor and grab and BEFORE the velocity, in list order,
 * one pass each, and never on a grabbed particle.  With p the position so far, prev the end of the previous substep and
 * dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z:
 *   sphere   d = p - a, L = sqrt(dot(d, d)); hit = L < radius && L > 0; n = d / L, depth = radius - L
 *   capsule  ab = b - a, t = dot(p - a, ab) / dot(ab, ab) (0 if dot(ab, ab) == 0), t = min(max(t, 0), 1); d = p - (a + ab*t),
 *            then as the sphere
 *   box      l_k = dot(p - a, axes[k]); hit iff |l_k| < b[k] for k = 0, 1, 2; k = the smallest b[k] - |l_k| (lowest k on ties);
 *            n = l_k >= 0 ? axes[k] : -axes[k], depth = b[k] - |l_k|
 *   plane    s = dot(p - a, b); hit = s < 0, n = b, depth = -s
 * and on a hit:  p = p + n*depth;  D = (prev - p) + velocity*dt;  T = D - n*dot(D, n);  p = p + T*min(1, dt*friction).
 * The plane y = 0 with normal (0, 1, 0), velocity 0 and the call's friction is the reference's floor.  Arithmetic: f32 in the
 * polar solver (PRECISE: no contraction, correctly rounded / and sqrt, the order above); Neo-Hookean PRECISE: f64 on the stored
 * f32 positions and the f64 collider values, p rounded to f32 after the push and again after the friction; FAST: f32 with
 * contraction and hardware reciprocals (tolerance level). */
enum { TETSIM_COLLIDER_SPHERE = 0, TETSIM_COLLIDER_CAPSULE = 1, TETSIM_COLLIDER_BOX = 2, TETSIM_COLLIDER_PLANE = 3 };
#define TETSIM_MAX_COLLIDERS 8
typedef struct TetSimCollider {
    int32_t kind;        /* TETSIM_COLLIDER_* */
    int32_t reserved;    /* must be 0 */
    double a[3];         /* sphere / box centre, capsule end A, a point on the plane */
    double b[3];         /* capsule end B; box half-extents; plane normal (points out of the solid) */
    double axes[9];      /* box only: its local x, y, z axes in world space (rows) */
    double radius;       /* sphere, capsule */
    double friction;     /* like physicsParams.friction: min(1, dt*friction) of the tangential slip is removed per contact */
    double velocity[3];  /* the collider's own velocity (m/s); friction acts on motion relative to it */
} TetSimCollider;
/* Replace the handle's list (count 0: none; colliders may then be NULL).  TETSIM_EINVAL, leaving the previous list in force, for:
 * count > TETSIM_MAX_COLLIDERS; an unknown kind or a non-zero `reserved`; a non-finite value in any field; a negative
 * radius, half-extent or friction; a zero-length plane normal or box axis; box axes that are not orthogonal (|u_i . u_j| > 1e-5
 * after normalisation).  Plane normals and box axes are normalised here in f64 (v / sqrt(v . v)); the f32 paths use the values
 * rounded once to f32. */
int tetsim_set_colliders(tetsim_handle h, const TetSimCollider *colliders, uint32_t count);

/* --- body grabs: one held particle per body of a batch, settable from device memory ------------- */

/* tetsim_set_grab holds ONE particle of the whole concatenation at a point in host memory.  The body-grab table holds one particle
 * of EVERY body (tetsim_create_batch; a single body is a batch of one), and a GPU-side loop can write it without the host.  An
 * ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look the symbols up.
 *
 * While body grabs are ON, particle first_particle[b] + particles[b] of body b is treated in every substep exactly as the particle
 * named by tetsim_set_grab is treated on that path: POLAR_JACOBI sets it to the target before the clamp, NEOHOOKEAN_GS after clamp
 * and floor, the colliders skip it.  Nothing else about a substep changes.  THE CONTRACT: body b of a batch with row (i, x) gives
 * the bits that body b created alone gives with tetsim_set_grab(i, x), for both solvers and both precisions, on every stepping
 * path.  A handle that never switches body grabs on executes what it always executed plus one uniform branch per particle pass.
 *
 * The table lives in device memory owned by the handle (num_bodies rows of 16 bytes and a body index per particle; it counts into
 * device_bytes).  The first set call allocates it with every row "none"; it is the only call that may block.  A set call writes
 * the table with one small kernel on the handle's stream, behind every substep enqueued so far; every substep enqueued afterwards
 * sees it.  tetsim_set_body_grabs_device follows the stream contract of tetsim_import_device: the handle's stream waits for
 * caller_stream, the kernel runs, caller_stream waits for the kernel; the host never reads the arrays and never synchronises.
 * Switching OFF (particles == NULL) is host state; it also puts every row back to "none".  The table is not solver state:
 * checkpoints and snapshots do not hold it, and their sizes do not change.
 *
 * Rows the host cannot see are normalised by the device kernel: a particle index outside [0, particles of body b) -- -1 is the
 * intended spelling -- or a non-finite target component makes THAT row "none" and disturbs no other body.  The host variant
 * refuses the same cases (other than -1) with TETSIM_EINVAL and leaves the table as it was.
 *
 * One kind of grab at a time: with body grabs ON, tetsim_set_grab(id >= 0), tetsim_start_grab and tetsim_start_grab_ray return
 * TETSIM_ESTATE (tetsim_set_grab(-1) stays legal); switching body grabs ON while a handle grab is set is TETSIM_ESTATE.  Also
 * TETSIM_ESTATE: any partitioned body; a handle with TETSIM_FLAG_REF_GRAB_TEXEL.  TETSIM_EINVAL: a NULL handle; NULL targets
 * with non-NULL particles; a stride that is neither 0 nor a multiple of 4 of at least 12; a pointer that is not 4-byte aligned,
 * that hipPointerGetAttributes does not place on the handle's device, or whose rows do not fit its allocation.  Every error is
 * found before anything is enqueued.
 * Cost, measured on an MI355X (tools/body_grabs_cost.py, profiles/body_grabs_cost.txt): never switched on, the benchmark
 * line is inside the parent's run-to-run spread; 64 Dragons in one batch with every body held against none held, one call of 20
 * substeps: polar FAST x1.20, Neo-Hookean FAST x0.99-1.02.
 * Out of scope: more than one grab per body (that is the pin table, tetsim_set_body_pins below); per-body parameters; partitioned
 * bodies; gradients; a Node binding. */

/* particles [num_bodies] int32: index INSIDE the body (0 = the body's first particle), -1 = this body is not held.
 * targets [num_bodies] rows of 3 f32.  particles == NULL: body grabs OFF (targets ignored). */
int tetsim_set_body_grabs(tetsim_handle h, const int32_t *particles, const float *targets);
/* The same from DEVICE memory: particles packed int32, targets rows of xyz f32 at targets + b * target_stride (0 = packed 12; else a
 * multiple of 4, >= 12), body_mask as for tetsim_snapshot_restore (num_bodies bytes, nonzero = take this body's row; NULL = all). */
int tetsim_set_body_grabs_device(tetsim_handle h, const void *particles, const void *targets, uint64_t target_stride,
                                 const void *body_mask, void *caller_stream);
/* The particle of every body nearest to a point, on the device: the counterpart of tetsim_nearest_particle / Grabber.start for a batch.
 * points: num_bodies rows of xyz f32 (stride 0 = packed 12).  ids [num_bodies] int32 packed: the body-local index of body b's particle
 * nearest to points[b]; dist2 [num_bodies] f64 packed, or NULL.  The squared distance is a0*a0 + a1*a1 + a2*a2 in f64 on the stored f32
 * positions of the last enqueued substep, without contraction; a NaN distance is never picked, the lowest index wins among equal
 * distances: id and dist2 are what tetsim_nearest_particle returns for body b alone in the same state, bit for bit.  A body with no
 * pickable particle gives -1 and DBL_MAX.  Two launches, no floating-point atomics: two calls give the same bits.  Stream contract and
 * pointer checks of tetsim_export_device (ids 4-byte, dist2 8-byte aligned); no host synchronisation; TETSIM_ESTATE for partitioned
 * bodies.  The ids it writes are directly the `particles` argument of tetsim_set_body_grabs_device. */
int tetsim_nearest_particles_device(tetsim_handle h, const void *points, uint64_t point_stride,
                                    void *ids, void *dist2, void *caller_stream);

/* --- body pins: many held particles per body of a batch, settable from device memory ------------- */

/* A body-grab row holds ONE particle of a body.  The pin table holds up to per_body particles of EVERY body, each at a target of its
 * own: a fixed base, a body hung from several points, a face clamped between gripper pads, boundary particles driven along a
 * trajectory.  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look the
 * symbols up.
 *
 * The table has num_bodies * per_body rows, body-major: row b * per_body + k is (particles[row], target xyz) -- a particle index
 * INSIDE body b, -1 = unused, and 3 f32.  While pins are ON, every particle a valid row names is treated in every substep, on every
 * stepping path, exactly as the particle named by tetsim_set_grab is treated on that path: POLAR_JACOBI sets it to its target before
 * the clamp, NEOHOOKEAN_GS after clamp and floor, the colliders skip it.  Nothing else about a substep changes.  THE CONTRACT: with
 * per_body = 1 a body gives the bits it gives with its body-grab row, and so those it gives alone with tetsim_set_grab; a body whose
 * every particle is pinned sits on its targets after every call, bit for bit.  A handle that never switches pins on executes what it
 * always executed: pins are a second mode of the body grabs' one uniform branch per particle pass, tested only behind it.
 *
 * NORMALISATION, the same for both variants and for tetsim_prep_pin_slots, in this order: (1) a row whose index is outside
 * [0, particles of body b) is "none"; (2) a row with a non-finite target component is "none"; (3) if two valid rows of one body
 * name the same particle, the LOWEST row wins and the later ones are ignored.  The device kernels apply all three silently and
 * disturb no other body.  The host variant refuses (1) -- other than -1 -- and (2) with TETSIM_EINVAL and leaves the previous
 * table in force; duplicates it accepts and resolves by (3).
 *
 * The table lives in device memory owned by the handle: an int32 per particle (the row that holds it, -1 = free) and 16 bytes per
 * row; it counts into device_bytes.  The first set call allocates it and may block.  A call with ANOTHER per_body than the table
 * has makes the rows anew: it waits for the handle's stream, may block, and empties every body's rows first -- a body that its
 * body_mask leaves out then holds nothing.  Every other set call only enqueues: on the handle's stream it clears the slots of the
 * bodies it takes, scatters the rows' indices with an integer atomicMin (the lowest row wins: two calls give the same bits; no
 * floating-point atomics) and writes the normalised rows; every substep enqueued afterwards sees them.  Switching OFF
 * (particles == NULL) is host state; it also empties the table.  The table is not solver state: checkpoints and snapshots do not
 * hold it, their sizes do not change, and a restore does not touch it.
 *
 * One kind of hold at a time: with pins ON, tetsim_set_grab(id >= 0), tetsim_start_grab, tetsim_start_grab_ray and switching body
 * grabs on return TETSIM_ESTATE (tetsim_set_grab(-1) stays legal); switching pins ON while a handle grab or body grabs are set is
 * TETSIM_ESTATE.  Also TETSIM_ESTATE: any partitioned body; a handle with TETSIM_FLAG_REF_GRAB_TEXEL.  TETSIM_EINVAL: a NULL
 * handle; NULL targets with non-NULL particles; per_body == 0 or per_body * num_bodies >= 2^31; and, for the device variant, a
 * stride that is neither 0 nor a multiple of 4 of at least 12; a pointer that is not 4-byte aligned, that hipPointerGetAttributes
 * does not place on the handle's device, or whose rows do not fit its allocation.  Every error is found before anything is
 * enqueued.
 * Cost, measured on an MI355X (tools/body_pins_cost.py, profiles/body_pins_cost.txt): never switched on, the benchmark
 * line is 34.04-34.15 G tet-solves/s against the parent's 33.88-34.12 in alternating runs -- no run below the parent's lowest, one
 * above its highest.  64 Dragons in one batch with 1 / 16 / 256 pins per body against none held, one call of 20 substeps: polar FAST
 * x1.20 / x1.22 / x1.16, Neo-Hookean FAST x0.99 / x1.01 / x1.01.  A body of the persistent 256-tet frame kernel (a single medium
 * body; TetSimInfo::fused_particle_pass == 2) leaves that kernel while pins are on and steps through its fused kernels, with the same
 * bits: a 28-cell lattice x1.68, whatever the number of pins.  The four-lane frame kernel of small bodies and the one-launch calls
 * keep their kernels.
 * Out of scope: pins on partitioned bodies; per-pin stiffness or springs (a pin is a hard hold); attachments between two bodies;
 * gradients; a Node binding. */

/* particles [num_bodies * per_body] int32, body-major: index INSIDE the body, -1 = unused row.  targets: a row of 3 f32 per row of
 * particles, packed.  particles == NULL: pins OFF (targets and per_body ignored). */
int tetsim_set_body_pins(tetsim_handle h, const int32_t *particles, const float *targets, uint32_t per_body);
/* The same from DEVICE memory: particles packed int32, targets rows of xyz f32 at targets + row * target_stride (0 = packed 12;
 * else a multiple of 4, >= 12); body_mask, the stream contract and the pointer checks are those of tetsim_set_body_grabs_device
 * (a body the mask leaves out keeps all its rows). */
int tetsim_set_body_pins_device(tetsim_handle h, const void *particles, const void *targets, uint64_t target_stride,
                                uint32_t per_body, const void *body_mask, void *caller_stream);
/* The normalisation above on the host, without a device: body_particles [num_bodies] particles of every body; slot_out
 * [sum of body_particles], in body order: for every particle the row (b * per_body + k) that holds it, -1 = free.  What the
 * device setter leaves in its slots, particle for particle.  TETSIM_EINVAL: a NULL argument, per_body == 0, per_body * num_bodies
 * >= 2^31. */
int tetsim_prep_pin_slots(const int32_t *particles, const float *targets, uint32_t num_bodies, uint32_t per_body,
                          const uint32_t *body_particles /*[num_bodies]*/, int32_t *slot_out /*[sum body_particles], -1 = free*/);

/* --- body colliders: up to eight colliders per body of a batch, settable from device memory ------ */

/* tetsim_set_colliders gives ONE list, from host memory, to every body of the handle.  The body-collider table gives EVERY body
 * (tetsim_create_batch; a single body is a batch of one) a list of its own -- a pusher, a jaw, a paddle, a tilted tray per
 * environment -- and a GPU-side loop can write it without the host.  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is
 * unchanged; no existing struct changed): look the symbols up.
 *
 * A row is TETSIM_BODY_COLLIDER_FLOATS f32, the fields of TetSimCollider in its order:
 *   [0] kind as a value (0.0 sphere, 1.0 capsule, 2.0 box, 3.0 plane; -1.0 = the slot is empty)   [1..3] a   [4..6] b   [7..15] axes
 *   [16] radius   [17] friction   [18..20] velocity   [21..23] never read
 * per_body (1 .. TETSIM_MAX_COLLIDERS) rows belong to each body, body-major: row (b, k) is row b * per_body + k.
 *
 * THE CONTRACT.  While body colliders are ON, a particle of body b meets the non-empty rows of body b, in slot order, exactly where and
 * how the handle's list acts on that path: after clamp, floor and grab, before the velocity, never on a held particle (held by
 * tetsim_set_grab or by the body's row of tetsim_set_body_grabs).  The arithmetic is the one defined above for tetsim_set_colliders.
 * Body b of a batch with rows r0 .. rk gives the bits that body b created alone gives with tetsim_set_colliders of the same rows
 * widened to double (every f32 is exactly a double), for both solvers, both precisions, every stepping path, tetsim_step and
 * tetsim_step_n.  A handle that never switches body colliders on executes what it always executed plus one uniform branch per
 * particle pass.  WHILE THEY ARE ON, the bodies whose call is one launch step through their stepwise kernels instead, which agree
 * with it bit for bit as they always have (TetSimInfo.fused_particle_pass keeps naming the body's own path): quad tiles
 * (fused_particle_pass 3) take two launches per substep, small Neo-Hookean bodies (4) a launch per level and body, clustered FAST
 * Neo-Hookean bodies a launch per colour.  Those one-launch kernels have no register for a second kind of list.
 *
 * The table lives in device memory owned by the handle: per body a count and up to eight compacted entries in the arithmetic view
 * the handle reads (f32 for POLAR_JACOBI and FAST NEOHOOKEAN_GS, f64 for PRECISE NEOHOOKEAN_GS), and the body index per particle it
 * shares with the body grabs; it counts into device_bytes.  The first set call allocates it with every body empty; it is the only
 * call that may block.  A set call writes the table with one small kernel (a lane per body) on the handle's stream, behind every
 * substep enqueued so far; every substep enqueued afterwards sees it.  Per row the kernel does what tetsim_set_colliders does on
 * the host: the same validity rules, the same f64 normalisation of the plane normal and the box axes, v / sqrt((v0*v0 + v1*v1) +
 * v2*v2), the same orthogonality test |u_i . u_j| > 1e-5, radius 0 for boxes and planes, the f32 view rounded once from the f64
 * view.  tetsim_set_body_colliders_device follows the stream contract of tetsim_import_device (the handle's stream waits for
 * caller_stream, the kernel runs, caller_stream waits for the kernel; the host never reads the rows and never synchronises).
 * Switching OFF (rows == NULL) is host state; it also empties every body.  The table is not solver state: checkpoints and
 * snapshots do not hold it, and their sizes do not change.
 *
 * Rows the host cannot see: a row tetsim_set_colliders would refuse -- a kind other than 0, 1, 2, 3 and -1; a non-finite value in
 * any of floats 0 .. 20; a negative radius, half-extent or friction; a zero normal or axis; axes that are not orthogonal -- becomes an
 * EMPTY SLOT.  It disturbs no other row and no other body, and the remaining rows keep their order.  A body the mask leaves out
 * keeps its whole list.  The host variant refuses the same cases (other than kind -1) with TETSIM_EINVAL, names the body and the
 * slot in tetsim_last_error, and leaves the table as it was.
 *
 * One kind of list at a time: with body colliders ON, tetsim_set_colliders with count > 0 returns TETSIM_ESTATE (count 0 stays
 * legal); switching body colliders ON while the handle's list is non-empty is TETSIM_ESTATE.  A shared obstacle goes into every
 * body's rows.  Also TETSIM_ESTATE: any partitioned body.  TETSIM_EINVAL: a NULL handle; per_body 0 or above TETSIM_MAX_COLLIDERS;
 * a stride that is neither 0 nor a multiple of 4 of at least 96; a pointer that is not 4-byte aligned, that hipPointerGetAttributes
 * does not place on the handle's device, or whose rows do not fit its allocation.  Every error is found before anything is enqueued.
 * Cost, measured on an MI355X (tools/body_colliders_cost.py, profiles/body_colliders_cost.txt): never switched on, the
 * benchmark line is inside the parent's run-to-run spread (32,676 .. 32,731 against 32,664 .. 32,811 M tet-solves/s, medians 32,685 and
 * 32,734) and pjb_call_kernel, pjb_frame_kernel and pjq_frame_kernel keep their registers (62, 162, 127; no scratch); 64 Dragons in
 * one batch, one call of 20 substeps, four colliders per body against the same four as the handle's list x1.01 (against none x1.37,
 * the list's own cost); one Dragon of quad tiles x1.76 and 64 small lattices of quad tiles x1.99 against the list (two launches per
 * substep); 64 Dragons Neo-Hookean FAST x207 (2.49 s against 12 ms: 43,520 level launches in place of one workgroup per body -- a
 * batch of small Neo-Hookean bodies pays dearly for the table); the set kernel takes 37 us for 64 bodies and 45 us for 4,096.
 * Out of scope: more than eight colliders per body; f64 rows; colliders
 * between bodies; partitioned bodies; a Node binding.  Contact read-back: tetsim_touch_bodies_device ("touch sensing", below). */
#define TETSIM_BODY_COLLIDER_FLOATS 24
/* rows: num_bodies * per_body rows of 24 f32, body-major (row of body b, slot k at index b * per_body + k), packed.
 * rows == NULL: body colliders OFF (per_body ignored). */
int tetsim_set_body_colliders(tetsim_handle h, const float *rows, uint32_t per_body);
/* The same from DEVICE memory: row (b, k) at rows + (b * per_body + k) * row_stride (0 = packed 96; else a multiple of 4, >= 96);
 * body_mask as for tetsim_set_body_grabs_device (num_bodies bytes, nonzero = take this body's rows; NULL = all). */
int tetsim_set_body_colliders_device(tetsim_handle h, const void *rows, uint64_t row_stride, uint32_t per_body,
                                     const void *body_mask, void *caller_stream);

/* --- body parameters: physics parameters per body of a batch, settable from device memory ------- */

/* Everything else that differs between the bodies of a batch already lives in per-body tables in device memory (grabs, colliders, poses,
 * resets); this table does the same for physicsParams: a stiff and a soft body, a slippery and a sticky floor, low gravity or another
 * arena for one environment, in ONE handle.  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing
 * struct changed): look the symbols up.
 *
 * A row is TETSIM_BODY_PARAMS_WIDTH f64, exactly a TetSimParams (sizeof == 80): gravity, friction, devCompliance, volCompliance,
 * worldBounds lo xyz, hi xyz.  f64 because PRECISE NEOHOOKEAN_GS reads the parameters as f64; the f32 view POLAR_JACOBI and FAST
 * NEOHOOKEAN_GS read is rounded once from the row, by the casts a call's TetSimParams goes through.
 *
 * THE CONTRACT.  While body parameters are ON, every substep of body b reads gravity, friction, devCompliance, volCompliance and
 * worldBounds from b's row.  The `params` argument of tetsim_step, tetsim_step_n and tetsim_profile must still be non-NULL; its values
 * are not looked at (as the handle's grab names nobody while body grabs are on).  dt stays the call's, for every body.  A
 * POLAR_JACOBI handle created with TETSIM_FLAG_REF_FIXED_BOUNDS keeps the reference's constant box for every body.  Body b gives the
 * bits it gives alone with those TetSimParams: both solvers, both precisions, every order, every stepping path, tetsim_step and
 * tetsim_step_n, with or without the handle's grab, body grabs, the handle's collider list and body colliders.  A handle that never
 * switches body parameters on executes what it always executed plus uniform branches on ONE flag (DevParams::body_params).
 *
 * Which kernel takes the table, per stepping path (TetSimInfo.fused_particle_pass): 0 POLAR_JACOBI gather / PRECISE -- pj_vertex_kernel,
 * per lane; 0 NEOHOOKEAN_GS levels, colours, clusters -- the level, cluster and particle kernels, per lane (tets through a tet -> body
 * array), and the one-launch clustered FAST sweeps nh_sweep1_kernel and nh_call_kernel likewise; 1 and 2 -- pjb_vertex_kernel per lane,
 * the fused tile kernel per tile (scalar loads); 3 -- pjq_frame_kernel and its two-launch twin, per tile (scalar loads); 2 / 3 with the
 * persistent pjb_frame_kernel -- per tile (scalar loads); 4 -- nh_frame_kernel, one workgroup per body (scalar loads); 5 --
 * pjb_call_kernel: tiles per tile, particle blocks per lane.  No path falls back to
 * other kernels while the table is on.
 *
 * The table lives in device memory owned by the handle, in the view its arithmetic reads (f32 or f64), with -- NEOHOOKEAN_GS -- the body
 * of every tet in the device's tet order; it counts into device_bytes.  The first set call allocates it with every body at
 * tetsim_default_params(); only that call may block.  A set call runs one small kernel, a lane per body, on the handle's stream, behind
 * every substep enqueued so far.  tetsim_set_body_params_device follows the stream contract of tetsim_import_device: no host read of
 * the rows, no host synchronisation.  A body the mask leaves out keeps its row.  Switching OFF (rows == NULL) is host state; the rows
 * stay.  The table is not solver state: checkpoints and snapshots do not hold it, and their sizes do not change.
 *
 * Rows the host cannot see: a row with a non-finite value in any of its ten doubles leaves its body's previous row in place and
 * disturbs no other body.  The host variant refuses such a row with TETSIM_EINVAL, names the body in tetsim_last_error and changes
 * nothing.  TETSIM_EINVAL also: a NULL handle; a stride that is neither 0 nor a multiple of 8 of at least 80; a pointer that is not
 * 8-byte aligned, not on the handle's device, or whose rows do not fit the allocation it points into; a mask with any of these faults.
 * TETSIM_ESTATE: any partitioned body.  Every error is found before anything is enqueued.
 * Cost, measured on an MI355X (tools/body_params_cost.py, profiles/body_params_cost.txt): never switched on, the benchmark
 * line is not below the parent's run-to-run range (medians 32,578.3 parent, 32,623.3 this change); switched on, 64 Dragons in one batch,
 * one call of 20 substeps: polar FAST x1.00, Neo-Hookean FAST x1.00 against the table off; the set kernel takes 32 us for 64 or 4,096 bodies.
 * Out of scope: per-body dt or density; a gravity vector; per-tet or per-particle material; partitioned bodies; a Node binding;
 * gradients. */
#define TETSIM_BODY_PARAMS_WIDTH 10   /* doubles per body row: 80 bytes, the fields of TetSimParams in its order */
enum { TETSIM_BP_GRAVITY = 0, TETSIM_BP_FRICTION = 1, TETSIM_BP_DEV_COMPLIANCE = 2, TETSIM_BP_VOL_COMPLIANCE = 3,
       TETSIM_BP_BOUNDS_LO = 4 /*..6*/, TETSIM_BP_BOUNDS_HI = 7 /*..9*/ };
/* rows: num_bodies rows of 10 f64, packed (an array of TetSimParams); rows == NULL: body parameters OFF */
int tetsim_set_body_params(tetsim_handle h, const double *rows);
/* The same from DEVICE memory: row b at rows + b * row_stride (0 = packed 80; else a multiple of 8, >= 80); body_mask as for
 * tetsim_set_body_grabs_device (num_bodies bytes, nonzero = take this body's row; NULL = all). */
int tetsim_set_body_params_device(tetsim_handle h, const void *rows, uint64_t row_stride, const void *body_mask, void *caller_stream);

/* --- device-side export and import: results for another GPU program, without a host copy -------- */

/* Whoever consumes the state on the device -- a PyTorch model, a renderer, a training loop that resets a batch of bodies -- gets it
 * in ITS memory, ordered against ITS stream; neither call synchronises the host.  An ADDITIVE extension of ABI version 5
 * (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look the symbols up.
 *
 * Rows and values are exactly what the matching host read returns, bit for bit, in the API's order (not the internal one), f32:
 *   TETSIM_FIELD_POSITIONS / _VELOCITIES / _PREV_POSITIONS   owned_particles rows of xyz: tetsim_read_positions / _velocities /
 *                                                            _prev_positions
 *   TETSIM_FIELD_QUATS                                       local_elems rows of xyzw in tetsim_get_local_tets order: tetsim_read_quats
 *                                                            (a TETSIM_FLAG_LEAN_STATE body recovers them first, on the device)
 *   TETSIM_FIELD_VISUAL_POSITIONS / _VISUAL_NORMALS          num_vis_verts rows of xyz: the two outputs of tetsim_read_visual_mesh
 *   TETSIM_FIELD_VISUAL_VERTEX_NORMALS                       num_vis_verts rows of xyz: tetsim_read_visual_vertex_normals
 * (the call skins, and computes the vertex normals, first; a batch is the concatenation, as everywhere).  Row r of a field goes to
 * dst + r * row_stride: 3 floats (QUATS: 4), and NOTHING else is written -- not the padding of a wider row, not a byte outside the
 * rows.  All fields of one call leave in one kernel launch.
 *
 * THE STREAM CONTRACT.  consumer_stream / producer_stream are hipStream_t values of the handle's device; 0 (NULL) is the legacy
 * default stream, which is what PyTorch uses unless told otherwise.  The handle steps on a non-blocking stream of its own, which
 * nothing orders against the caller's streams but these two calls:
 *   tetsim_export_device  (1) records an event on consumer_stream and (2) makes the handle's stream wait for it -- whatever the
 *     caller enqueued earlier that still reads or writes `dst` is done before the export writes; (3) enqueues the export on the
 *     handle's stream, behind every substep enqueued so far; (4) records an event there and makes consumer_stream wait for it.
 *     After the call returns, work the caller enqueues on consumer_stream sees the data; substeps enqueued on the handle afterwards do
 *     not disturb it (they never touch `dst`).  Work on OTHER streams of the caller needs the caller's own ordering against
 *     consumer_stream.
 *   tetsim_import_device  (1) the handle's stream waits for an event recorded on producer_stream -- `pos` and `vel` are complete;
 *     (2) one kernel writes the state, behind every substep enqueued so far; (3) producer_stream waits for that kernel, so the
 *     caller may reuse or free `pos` and `vel` in stream order.
 * The events live in the handle (created by the first such call, destroyed by tetsim_destroy).  Only that first call of a handle may
 * block: it allocates them and, for a body with an internal particle order, uploads the index map once.
 *
 * tetsim_import_device leaves the state tetsim_write_state leaves for the same numbers: pos / vel [owned_particles] rows of xyz, the
 * inverse masses kept; POLAR_JACOBI predicts afresh at the next step; per-tet state (quaternions, carried shape) is untouched.
 * pos_stride / vel_stride follow the rule of row_stride below.
 *
 * Every error is found before anything is enqueued and leaves `dst` and the state as they were.  TETSIM_EINVAL: a NULL handle,
 * `fields`, `dst`, `pos` or `vel`; count == 0 or count > TETSIM_MAX_EXPORT_FIELDS; an unknown field; reserved != 0; a stride that is
 * neither 0 nor a multiple of 4 of at least the row's bytes; a pointer that is not 4-byte aligned, that hipPointerGetAttributes does
 * not report as device memory of the handle's device, or whose rows do not fit the allocation it points into.  TETSIM_ESTATE: QUATS or
 * VISUAL_NORMALS on a NEOHOOKEAN_GS body (VISUAL_NORMALS also needs the rest normals of tetsim_set_visual_mesh); PREV_POSITIONS on
 * a POLAR_JACOBI body; a visual field without a visual mesh, VISUAL_VERTEX_NORMALS without triangles; any partitioned body (its halo
 * stream and ghosts need a contract of their own).
 * Out of scope: partitioned bodies; element types other than f32; gradients. */
enum { TETSIM_FIELD_POSITIONS = 0, TETSIM_FIELD_VELOCITIES = 1, TETSIM_FIELD_PREV_POSITIONS = 2,
       TETSIM_FIELD_QUATS = 3, TETSIM_FIELD_VISUAL_POSITIONS = 4, TETSIM_FIELD_VISUAL_NORMALS = 5,
       TETSIM_FIELD_VISUAL_VERTEX_NORMALS = 6 };
#define TETSIM_MAX_EXPORT_FIELDS 8
typedef struct TetSimDeviceField {
    int32_t field, reserved;   /* reserved must be 0 */
    void *dst;                 /* DEVICE memory of the handle's device, 4-byte aligned */
    uint64_t row_stride;       /* bytes between rows; 0 = packed (12, QUATS 16); otherwise >= row bytes and a multiple of 4 */
} TetSimDeviceField;
int tetsim_export_device(tetsim_handle h, const TetSimDeviceField *fields, uint32_t count, void *consumer_stream);
int tetsim_import_device(tetsim_handle h, const void *pos, uint64_t pos_stride,
                         const void *vel, uint64_t vel_stride, void *producer_stream);

/* --- device snapshots: the complete state kept in device memory, captured and restored for chosen bodies -------- */

/* tetsim_import_device writes positions and velocities; the per-tet state of a POLAR_JACOBI body (quaternion, carried shape) stays.  The
 * complete restore used to be tetsim_save_state / tetsim_load_state alone: through host memory, behind a drain of the queues, for every
 * body of the handle.  A SNAPSHOT is that same state -- every section a checkpoint holds, one device buffer each; not a second copy of
 * the constant tables -- kept in device memory, and restored for the bodies a device-side mask names: an episode loop over a batch resets
 * environments 3 and 17 and leaves the other 62 alone, without a host synchronisation.  An ADDITIVE extension of ABI version 5
 * (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look the symbols up.
 *
 *   tetsim_snapshot_create   allocates the buffers (they count into TetSimInfo.device_bytes) and captures the current state of all
 *                            bodies, on the handle's stream behind every substep enqueued so far.  It may block: it allocates.
 *   tetsim_snapshot_capture  overwrites the chosen bodies' part of the snapshot with their current state.
 *   tetsim_snapshot_restore  overwrites the chosen bodies' current state with their part of the snapshot.
 *   tetsim_snapshot_destroy  waits for the handle's stream and frees the buffers; NULL is harmless.  A snapshot belongs to the handle
 *                            that created it, and tetsim_destroy frees the snapshots that are left (their pointers die with it).
 *
 * body_mask is DEVICE memory of the handle's device: TetSimInfo.num_bodies bytes, nonzero = chosen (the layout of a torch.bool
 * tensor); NULL = all bodies (a single body: NULL or a one-byte mask).  The host never reads it.
 *
 * THE STREAM CONTRACT is that of tetsim_import_device: (1) the handle's stream waits for an event recorded on caller_stream -- the mask
 * is complete before it is read; (2) ONE kernel moves every section, behind every substep enqueued so far; (3) caller_stream waits for
 * that kernel, so the caller may overwrite or free the mask in stream order.  Neither capture nor restore synchronises the host.  Only
 * the first such call of a handle may block: it creates the events (the export's and import's) and, with a mask, uploads the table that
 * tells every row's body.
 *
 * WHAT A RESTORE LEAVES.  With a NULL mask exactly what tetsim_load_state leaves for a blob saved at the moment of the capture, bit for
 * bit, in every section, the predictions and the recorded dt included.  The fourth float of the rows that carry a call's sequence number
 * (POLAR_JACOBI predictions and end-of-substep positions, NEOHOOKEAN_GS previous positions) holds 0, as in a checkpoint: the kernel
 * clears it on the way in and on the way out.  A TETSIM_FLAG_LEAN_STATE body recovers its quaternions on its stream before a capture
 * (no host wait), so a snapshot's quaternions are the ones its shapes give; recovering them again from the same shape next to the
 * quaternion stored there gives the same bits, so a masked restore needs no recovery of its own and leaves the "stale" mark as it was.
 * With a mask the rows of the bodies not chosen are not written at all.
 *
 * FOR WHICH dt THE PREDICTIONS HOLD is host-side state (POLAR_JACOBI) and does not depend on the mask's contents.  The snapshot records
 * it at every capture: a NULL-mask capture records the handle's, a masked one the intersection of its record and the handle's.  A masked
 * restore leaves the handle with the intersection of its own and the snapshot's; a NULL-mask restore with the snapshot's.  "Valid for
 * any dt" (no substep yet: the velocities are zero) intersected with X is X; two different dt have nothing in common, and then the next
 * step predicts every particle afresh, as after tetsim_import_device.  A snapshot taken right after creation, or a loop that keeps dt
 * fixed, never gets there, and then the bodies not chosen are untouched bit for bit.  In the empty case they get pos + vel * dt from the
 * re-prediction kernel in place of the prediction they carried (made with the dt of their last substep: the new dt makes every
 * prediction stale, restore or not).  That kernel and the gather formulation's particle kernel compute the same expression, a product
 * and a sum (PRECISE: the same bits); the blocked formulation's particle kernels (FAST, the default) use one fused multiply-add where the
 * re-prediction kernel rounds twice, so there a re-predicted value can differ from the particle kernel's in the last bit.
 *
 * Every error is found before anything is enqueued and leaves the state and the snapshot as they were.  TETSIM_EINVAL: a NULL handle,
 * snapshot or `out`; a snapshot of another handle; a mask that hipPointerGetAttributes does not report as device memory of the handle's
 * device, or whose allocation holds fewer than num_bodies bytes from that pointer.  TETSIM_ESTATE: any partitioned body.
 * Out of scope: partitioned bodies; per-body parameters; the body-grab table (tetsim_set_body_grabs: a restore does not touch it); snapshots shared between handles; a
 * snapshot in caller-owned memory. */
typedef struct tetsim_snapshot_s *tetsim_snapshot;
int tetsim_snapshot_create(tetsim_handle h, tetsim_snapshot *out);
int tetsim_snapshot_capture(tetsim_handle h, tetsim_snapshot s, const void *body_mask, void *caller_stream);
int tetsim_snapshot_restore(tetsim_handle h, tetsim_snapshot s, const void *body_mask, void *caller_stream);
void tetsim_snapshot_destroy(tetsim_snapshot s);

/* --- placement: a rigid motion of chosen bodies' complete state, rows and mask in device memory -------- */

/* A restore puts a body back exactly where the snapshot found it; tetsim_import_device writes positions and velocities and leaves a
 * POLAR_JACOBI body's per-tet state (quaternion, carried shape) behind.  A PLACEMENT starts an episode somewhere else: every chosen body
 * b of the handle gets ONE rigid motion, applied to the COMPLETE state -- every section a checkpoint or a snapshot holds -- so that the
 * body continues as a body that had always been there: randomised start poses, a drop from a new height and orientation, a throw with a
 * linear and an angular velocity, one environment moved out of another's way.  An ADDITIVE extension of ABI version 5
 * (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look the symbols up.
 *
 * A body's row is TETSIM_PLACE_WIDTH f32: Q (xyzw, any length but 0), PIVOT, OFFSET, LINEAR, ANGULAR (xyz each).  body_mask is as for
 * tetsim_snapshot_restore: num_bodies bytes, nonzero = chosen; NULL = all.
 *
 * DEFINITION.  All arithmetic is f64 on the stored f32 values, every operation rounded on its own (no fused multiply-add); results are
 * stored as f32 (f32(.) below).  cross is the observations' (above).
 *   n = sqrt(((qx*qx + qy*qy) + qz*qz) + qw*qw)        (x,y,z,w) = Q / n, component by component
 *   with xx = x*x, xy = x*y, ... :   m00 = 1 - 2*(yy+zz)   m01 = 2*(xy - wz)     m02 = 2*(xz + wy)
 *                                    m10 = 2*(xy + wz)     m11 = 1 - 2*(xx+zz)   m12 = 2*(yz - wx)
 *                                    m20 = 2*(xz - wy)     m21 = 2*(yz + wx)     m22 = 1 - 2*(xx+yy)
 *   Rot(d)_i = (m_i0*d.x + m_i1*d.y) + m_i2*d.z          c = PIVOT + OFFSET
 *   positions        r = Rot(p - PIVOT)     p' = f32(r + c)        (NEOHOOKEAN_GS: the previous positions by the same rule)
 *   velocities       u = LINEAR + cross(ANGULAR, r)     v' = f32(u), or with TETSIM_PLACE_KEEP_VELOCITY  v' = f32(Rot(v) + u)
 *   quaternions      (POLAR_JACOBI)  q' = f32(qR (x) q), qR = (x,y,z,w), the product in the reference's term order
 *                    (SoftbodyGPU.js:114-121: q'.x = ((w1*x2 + x1*w2) + y1*z2) - z1*y2, ...); it is not renormalised
 *   carried shape    (POLAR_JACOBI)  a layout of world-space corners, as the reference's textureElem (the gather formulation): every
 *                    corner e' = f32(Rot(e - PIVOT) + c).  A layout of corners relative to their own centroid (the blocked formulation:
 *                    four corners, or the three of TETSIM_FLAG_LEAN_STATE): e' = f32(Rot(e)).  Constant-rest-shape bodies carry none.
 *   The fourth float of every 16-byte row (inverse volume, inverse mass, sequence numbers) is left as it is; NEOHOOKEAN_GS volError is
 *   untouched.
 *   predictions      (POLAR_JACOBI) are state: the chosen bodies are left with pos' + vel' * dt in the re-prediction kernel's arithmetic
 *                    (f32: a product, then a sum), dt the one the handle's predictions were made with.  The bodies not chosen are not
 *                    written at all: with a fixed dt they continue bit for bit.  While the handle's predictions are "valid for any dt"
 *                    (no substep yet) the call marks them stale for the whole handle instead: the next step predicts every particle
 *                    afresh, which gives a particle of zero velocity its position back.
 * A TETSIM_FLAG_LEAN_STATE body first brings its stored quaternions up to date on its stream, as a snapshot capture does (no host
 * wait), then turns shape and quaternion together: the recovery's sign rule keeps seeing a consistent pair.
 *
 * A row with a non-finite value or with n == 0 leaves ITS body alone and untouched and disturbs no other, as a row the grab table cannot
 * hold does; the host variant refuses the same rows of chosen bodies with TETSIM_EINVAL and changes nothing.
 *
 * THE STREAM CONTRACT is that of tetsim_import_device: (1) the handle's stream waits for an event recorded on caller_stream -- rows and
 * mask are complete; (2) ONE kernel moves every section, behind every substep enqueued so far; (3) caller_stream waits for it, so the
 * caller may reuse rows and mask in stream order.  No host synchronisation; only a handle's first call may block (it uploads the table
 * that tells every row's body, the snapshots' own; the host variant allocates where its rows wait, num_bodies * 65 bytes that count
 * into device_bytes).  The host variant copies rows and mask during the call, enqueues the same kernel and does not wait for it.
 *
 * Every error is found before anything is enqueued and leaves the state as it was.  TETSIM_EINVAL: a NULL handle or rows; flag bits
 * other than TETSIM_PLACE_KEEP_VELOCITY; a row_stride that is neither 0 (packed: 64) nor a multiple of 4 of at least 64; rows that are
 * not 4-byte aligned, that hipPointerGetAttributes does not report as device memory of the handle's device, or that do not fit the
 * allocation they point into; such a mask.  TETSIM_ESTATE: any partitioned body.
 * The grab tables, the collider list, snapshots and checkpoints are untouched; a checkpoint saved after a placement holds the placed
 * state.  A POLAR_JACOBI velocity already holds the next substep's gravity * dt (SoftbodyGPU.js:369-371), and KEEP_VELOCITY turns it
 * with the rest.  The world clamp and the floor act at the next substep as always.
 * Cost, measured on an MI355X: tools/place_cost.py, profiles/place_cost.txt.
 * Out of scope: partitioned bodies; per-body scaling or shear; a Node binding; gradients; placement relative to the mass centre (the
 * caller passes TETSIM_OBS_COM of tetsim_observe_bodies_device as PIVOT). */
#define TETSIM_PLACE_WIDTH 16            /* floats per body row: 64 bytes */
enum { TETSIM_PLACE_Q = 0 /*..3 xyzw*/, TETSIM_PLACE_PIVOT = 4 /*..6*/, TETSIM_PLACE_OFFSET = 7 /*..9*/,
       TETSIM_PLACE_LINEAR = 10 /*..12*/, TETSIM_PLACE_ANGULAR = 13 /*..15*/ };
enum { TETSIM_PLACE_KEEP_VELOCITY = 1u << 0 };
/* rows, body_mask: DEVICE memory of the handle's device; row b at rows + b*row_stride (0 = packed 64; else a multiple of 4, >= 64) */
int tetsim_place_bodies_device(tetsim_handle h, const void *rows, uint64_t row_stride,
                               const void *body_mask, uint32_t flags, void *caller_stream);
/* the same from HOST memory: rows [num_bodies*16] packed, mask num_bodies bytes or NULL */
int tetsim_place_bodies(tetsim_handle h, const float *rows, const uint8_t *body_mask, uint32_t flags);

/* --- per-body observations on the device: mass centre, bounds, volume, tet health -------- */

/* What decides which bodies of a batch to reset: where each body is, how fast, whether it left the arena, whether a tet turned inside
 * out -- one row of TETSIM_OBS_WIDTH doubles per body, in the caller's DEVICE memory, with no host synchronisation (or, through
 * tetsim_read_body_observations, the same rows on the host).  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged;
 * no existing struct changed): look the symbols up.
 *
 * DEFINITIONS.  All arithmetic is f64 on the stored f32 values (what tetsim_read_positions / _velocities return), every operation rounded
 * on its own (no fused multiply-add).  dot(u,v) = (u.x*v.x + u.y*v.y) + u.z*v.z; cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 * a.x*b.y - a.y*b.x).  Per tet with corners 0..3 in the caller's numbering (a batch: the concatenation), r_k the rest positions given at
 * creation, x_k / v_k the current positions / velocities:
 *   V0 = dot(r1-r0, cross(r2-r0, r3-r0)) / 6   computed once on the host; it KEEPS ITS SIGN, as the reference's initPhysics does
 *   w  = (density * V0) / 4                    a quarter of the tet's mass for each corner.  This is the observation's own f64 definition of
 *                                              the lumped mass: NOT the f32 invMass that Softbody.js:74-78 accumulates add by add
 *                                              (tetsim_read_inv_mass), from which it differs in the last bits
 *   V  = dot(x1-x0, cross(x2-x0, x3-x0)) / 6
 * and per body, summed over its tets (S = sum):
 *   MASS = S 4w      COM = (S w * (((x0+x1)+x2)+x3)) / MASS      VCOM = (S w * (((v0+v1)+v2)+v3)) / MASS      (3 doubles each)
 *   VOLUME = S V     REST_VOLUME = S V0
 *   MIN_VOLUME_RATIO = min V/V0 over the tets with V0 != 0 (+inf if there is none; a NaN ratio is left out, see NONFINITE)
 *   INVERTED_TETS    = the number of those tets with V/V0 <= 0
 *   a body with MASS == 0 (no tets) reports COM = VCOM = 0
 * and over its particles:
 *   AABB_MIN / AABB_MAX = the box of the positions (3 doubles each)      MAX_SPEED2 = max (vx*vx + vy*vy) + vz*vz
 *   NONFINITE = the number of particles with a non-finite component in position or velocity.  Those particles are left out of the box
 *   and of MAX_SPEED2; the tet sums are NOT filtered, so a NaN shows in COM.  A body without a finite particle reports +inf / -inf as
 *   its box and 0 as MAX_SPEED2.
 * Counts are reduced as integers and stored as doubles.  RESERVED is written as 0.
 *
 * REPRODUCIBLE AND POSITION INDEPENDENT.  A body's tets and particles are cut into chunks of 256 counted from the body's own first tet /
 * particle, a chunk is reduced by a fixed tree, and the chunks' partial rows are reduced in index order by the same tree; there are no
 * floating-point atomics.  So two calls on the same state give the same bits, and a body of a batch gives the bits the same body gives
 * alone in the same state.  Nothing depends on a stepping path's internal particle or tet order.
 *
 * Row b of dst = body b of the handle (tetsim_get_batch_layout), at dst + b * row_stride; only the TETSIM_OBS_WIDTH doubles of a row
 * are written -- not the padding of a wider row, not a byte outside the rows.  THE STREAM CONTRACT is that of tetsim_export_device:
 * the handle's stream waits for caller_stream, two launches run behind every substep enqueued so far, caller_stream waits for them.
 * Only the handle's first observation may block: it builds the constant per-tet table (ids and V0, 24 bytes per tet) on the host and
 * uploads it with the scratch of the partial rows -- and the handle's two chunk tables (12 bytes per chunk of 256 tets / particles, 8 per
 * body; shared with the pose, strain and nearest-particle calls, uploaded once by whichever of them comes first); all of it counts into
 * TetSimInfo.device_bytes from then on.
 * tetsim_read_body_observations writes the same rows to host memory, out[num_bodies * TETSIM_OBS_WIDTH], and synchronises.
 *
 * Every error is found before anything is enqueued and leaves `dst` as it was.  TETSIM_EINVAL: a NULL handle, dst or out; a dst that
 * is not 8-byte aligned; a row_stride that is neither 0 (packed: 160) nor a multiple of 8 of at least 160; a dst that
 * hipPointerGetAttributes does not report as device memory of the handle's device, or whose rows do not fit the allocation it points
 * into.  TETSIM_ESTATE: a partitioned body.
 * Out of scope: partitioned bodies; energies; per-tet output fields; a body mask; thresholds or "done" flags (the caller compares). */
#define TETSIM_OBS_WIDTH 20          /* doubles per body row: 160 bytes */
enum { TETSIM_OBS_MASS = 0, TETSIM_OBS_COM = 1 /*..3*/, TETSIM_OBS_VCOM = 4 /*..6*/, TETSIM_OBS_VOLUME = 7,
       TETSIM_OBS_REST_VOLUME = 8, TETSIM_OBS_MIN_VOLUME_RATIO = 9, TETSIM_OBS_INVERTED_TETS = 10,
       TETSIM_OBS_AABB_MIN = 11 /*..13*/, TETSIM_OBS_AABB_MAX = 14 /*..16*/, TETSIM_OBS_MAX_SPEED2 = 17,
       TETSIM_OBS_NONFINITE = 18, TETSIM_OBS_RESERVED = 19 /* written as 0 */ };
/* row b of dst (DEVICE memory, f64) = body b of the handle; ordered against caller_stream exactly as tetsim_export_device */
int tetsim_observe_bodies_device(tetsim_handle h, void *dst, uint64_t row_stride, void *caller_stream);
/* the same rows into host memory [num_bodies * TETSIM_OBS_WIDTH]; synchronises */
int tetsim_read_body_observations(tetsim_handle h, double *out);

/* --- per-body pose on the device: best-fit rotation, angular velocity, rigid-fit residual ------- */

/* Which way up a body is and how it spins: the other half of the rigid state whose first half (mass centre and its velocity) the
 * observation row holds, and the inverse of tetsim_place_bodies_device -- place a rest body by Q and its pose row reports +-Q.  One row of
 * TETSIM_POSE_WIDTH doubles per body, in the caller's DEVICE memory, with no host synchronisation (or, through tetsim_read_body_poses,
 * the same rows on the host).  A read-only query: no solver state changes.  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION
 * is unchanged; no existing struct changed): look the symbols up.
 *
 * THE TABLE.  Built once on the host in f64, every operation rounded on its own; tetsim_prep_pose_table returns the same values.  With
 * the observation's V0 and w = (density * V0) / 4 (above, sign kept) and r_i the f32 rest positions:
 *   m_i = the sum of w over the corners that name particle i, tets in ascending index, corners 0..3 of a tet in that order, from 0.0
 *   per body, over its own particles in ascending index, from 0.0:  M0 = S m_i,  c0 = (S m_i * r_i) / M0 component by component,
 *   c0 = 0 if M0 == 0;   q_i = r_i - c0.
 * A particle's record is { double m, qx, qy, qz }, 32 bytes.
 *
 * THE ROW, PART 1: RAW MOMENTS [0..25].  Sums (S) over the body's particles; x, v the stored f32 positions and velocities, m, q the
 * table's; f64, every operation rounded on its own (no fused multiply-add); dot and cross are the observations'.
 *   [0]      MASS = S m                [1..3]   MX = S m*x            [4..6]   MV = S m*v
 *   [7..15]  A, row-major: A_ab = S (m*x_a)*q_b                      (at 7 + 3*a + b)
 *   [16..18] L0 = S m*cross(x, v)      component by component: m * (x.y*v.z - x.z*v.y), ...
 *   [19..24] G = S (m*x_a)*x_b for ab = xx, yy, zz, xy, xz, yz
 *   [25]     Q0 = S m*dot(q, q)
 * Nothing is filtered: a non-finite particle shows as NaN in its own body's sums and in no other body's.  The reduction is the
 * observations': a body's particles are cut into chunks of 256 counted from its own first particle, a fixed tree reduces inside a chunk
 * (lane l takes lane l + 32, 16, .. 1 within a wave of 64, then the four waves as (w0 + w1) + (w2 + w3)), the chunks' rows are reduced
 * in index order by the same tree (thread t folds rows t, t + 256, .. in that order, from 0.0), and there are no floating-point
 * atomics.  So two calls give the same bits, and a body of a batch gives the bits it gives alone.
 *
 * THE ROW, PART 2: DERIVED VALUES [26..47].  A fixed f64 procedure on the STORED raw values [0..25] and nothing else, with only
 * + - * / sqrt, comparisons, fabs and negation, every operation rounded on its own and every sum in the order of its parentheses:
 * tests/pose_ref.py reproduces [26..47] bit for bit in numpy from a row's own [0..25].  (x, y, z = components 0, 1, 2.)
 *   MASS == 0:  COM = VCOM = OMEGA = L = 0, Q = (0,0,0,1), RESIDUAL = GAP = 0, and nothing below is evaluated.  Otherwise:
 *   [26..28] COM_a = MX_a / MASS                       [29..31] VCOM_a = MV_a / MASS
 *   [39..41] L = L0 - cross(COM, MV):   L.x = L0.x - (COM.y*MV.z - COM.z*MV.y), ...          the angular momentum about the mass centre
 *            Gc_ab = G_ab - (MX_a*MX_b)/MASS  (the six of G)       T = (Gc_xx + Gc_yy) + Gc_zz
 *            Ic (symmetric):  Ixx = T - Gc_xx, Iyy = T - Gc_yy, Izz = T - Gc_zz, Ixy = -Gc_xy, Ixz = -Gc_xz, Iyz = -Gc_yz
 *            its adjugate:    a00 = Iyy*Izz - Iyz*Iyz    a01 = Ixz*Iyz - Ixy*Izz    a02 = Ixy*Iyz - Ixz*Iyy
 *                             a11 = Ixx*Izz - Ixz*Ixz    a12 = Ixy*Ixz - Ixx*Iyz    a22 = Ixx*Iyy - Ixy*Ixy
 *            det = (Ixx*a00 + Ixy*a01) + Ixz*a02
 *   [36..38] OMEGA = (adj * L) / det:   OMEGA.x = ((a00*L.x + a01*L.y) + a02*L.z) / det,  .y = ((a01*L.x + a11*L.y) + a12*L.z) / det,
 *            .z = ((a02*L.x + a12*L.y) + a22*L.z) / det;   det == 0 gives OMEGA = 0                Ic * OMEGA = L
 *   [32..35] Q (x,y,z,w): the proper rotation R that minimises S m |R q - (x - COM)|^2 (Horn's absolute-orientation quaternion; a
 *            mirrored body gets its best proper rotation, not a reflection).  With S_ab = A_ba -- the term (MX_a * S m*q_b) / MASS of
 *            the centred moment is DROPPED: S m*q is 0 up to the rounding of the table and is not part of the row -- the symmetric
 *              N00 = (Sxx + Syy) + Szz    N01 = Syz - Szy            N02 = Szx - Sxz            N03 = Sxy - Syx
 *                                         N11 = (Sxx - Syy) - Szz    N12 = Sxy + Syx            N13 = Szx + Sxz
 *                                                                    N22 = (Syy - Sxx) - Szz    N23 = Syz + Szy
 *                                                                                               N33 = (Szz - Sxx) - Syy
 *            is diagonalised by the Jacobi procedure below with V = I accumulating the rotations.  k = the index of the largest diagonal
 *            entry (found by ascending scan with >, so ties go to the lower index and a NaN leaves k = 0), lambda_max = N_kk,
 *            (w,x,y,z) = column k of V, divided component by component by n = sqrt(((w*w + x*x) + y*y) + z*z).  The sign: all four are
 *            negated if w < 0, or if w == 0 and the first non-zero of x, y, z is negative.
 *   [42]     RESIDUAL = sqrt(e < 0 ? 0 : e),  e = ((T + Q0) - 2*lambda_max) / MASS       the rms distance, in metres, to the best rigid fit
 *   [43]     GAP = lambda_max - the largest of the other three diagonal entries (ascending scan with >, from the first of them).
 *            Small against lambda_max: the orientation is ill-defined (flat, collinear, mirrored shapes, a half turn away from a tie)
 *   [44..47] RESERVED, written as 0
 *
 * THE JACOBI PROCEDURE is the strain section's (below), extended to 4x4 with eigenvectors: TETSIM_POSE_SWEEPS cyclic sweeps over the
 * pairs (0,1), (0,2), (0,3), (1,2), (1,3), (2,3), no convergence test.  For a pair (p,q): nothing if N_pq == 0; otherwise theta, t, c, s
 * by the strain section's formulas from N_pp, N_qq, N_pq, then
 *   N_pp -= t*N_pq    N_qq += t*N_pq    N_pq = 0    for the two other indices r (ascending): (N_rp, N_rq) <- (c*N_rp - s*N_rq, s*N_rp + c*N_rq)
 *   for the four rows k of V:  (V_kp, V_kq) <- (c*V_kp - s*V_kq, s*V_kp + c*V_kq)
 * WHY 5 SWEEPS.  It is the smallest count at which tests/pose_ref.py agrees with numpy.linalg.eigh on the inputs of
 * tests/test_pose_cpu.py (4,000 seeded moment sets -- generic, flat, collinear, mirrored, half turns (w = 0), far from the origin -- and
 * the stepped Dragon states of tests/golden) within that test's margin: d = (48 * sweeps + 16) * 2^-53 * ||N||_F for lambda_max,
 * 2 * d for GAP and d / GAP for the quaternion (up to sign; sets whose d / GAP exceeds 1e-3 -- the collinear ones -- must report that
 * small a GAP instead).  Observed at 5 sweeps: 0.033 of the margin at worst for lambda_max, 0.016 for GAP, 0.027 for the quaternion, and
 * less than 4e-18 * ||N||_F left off the diagonal; at 4 sweeps 6.9e6 times the margin (not converged).
 * PRECISION.  The moments are taken about the ORIGIN (one pass, no second read of the particles): A, G and L0 carry rounding errors of
 * about n * 2^-53 * |COM| * |q| per unit mass against a signal of |q|^2, so the rotation loses |COM| / |q| of f64's sixteen digits and
 * RESIDUAL, a difference of sums, has a floor of about sqrt(n * 2^-53) * |COM|.  A body a kilometre from the origin still has nine
 * digits of orientation.
 *
 * Row b of dst = body b of the handle (tetsim_get_batch_layout), at dst + b * row_stride; only the TETSIM_POSE_WIDTH doubles of a row
 * are written -- not the padding of a wider row, not a byte outside the rows.  THE STREAM CONTRACT is that of
 * tetsim_observe_bodies_device: the handle's stream waits for caller_stream, two launches run behind every substep enqueued so far,
 * caller_stream waits for them.  Only the handle's first pose call may block: it builds the table on the host and uploads it (32 bytes
 * per particle) with the scratch of the chunk rows (26 doubles per chunk of 256 particles), the rows of the host read and, unless an
 * observation or a nearest-particle call made it, the handle's particle chunk table (the observation's; never the tet one); all of it
 * counts into TetSimInfo.device_bytes from then on.  tetsim_read_body_poses writes the same rows to host memory,
 * out[num_bodies * TETSIM_POSE_WIDTH], and synchronises.
 * THE KERNELS.  One lane per particle, 256 per workgroup: a 32-byte record and two gathered 16-byte rows, 96 bytes per particle, 26
 * f64 accumulators per lane; one workgroup per body folds the chunk rows, and its first lane runs the derived procedure on the values
 * it just stored.  Cost, measured on an MI355X against the observation: tools/pose_cost.py, profiles/pose_cost.txt.
 *
 * Every error is found before anything is enqueued and leaves `dst` as it was.  TETSIM_EINVAL: a NULL handle, dst or out; a dst that
 * is not 8-byte aligned; a row_stride that is neither 0 (packed: 384) nor a multiple of 8 of at least 384; a dst that
 * hipPointerGetAttributes does not report as device memory of the handle's device, or whose rows do not fit the allocation it points
 * into.  TETSIM_ESTATE: a partitioned body.
 * Out of scope: partitioned bodies; a body mask; a Node binding; gradients; the inertia in the body's frame; filtering non-finite
 * particles. */
#define TETSIM_POSE_WIDTH 48         /* doubles per body row: 384 bytes */
#define TETSIM_POSE_SWEEPS 5         /* cyclic Jacobi sweeps behind Q */
enum { TETSIM_POSE_MASS = 0, TETSIM_POSE_MX = 1 /*..3*/, TETSIM_POSE_MV = 4 /*..6*/, TETSIM_POSE_A = 7 /*..15, row-major*/,
       TETSIM_POSE_L0 = 16 /*..18*/, TETSIM_POSE_G = 19 /*..24: xx yy zz xy xz yz*/, TETSIM_POSE_Q0 = 25,
       TETSIM_POSE_COM = 26 /*..28*/, TETSIM_POSE_VCOM = 29 /*..31*/, TETSIM_POSE_Q = 32 /*..35 xyzw*/, TETSIM_POSE_OMEGA = 36 /*..38*/,
       TETSIM_POSE_L = 39 /*..41*/, TETSIM_POSE_RESIDUAL = 42, TETSIM_POSE_GAP = 43, TETSIM_POSE_RESERVED = 44 /*..47, written as 0*/ };
/* row b of dst (DEVICE memory, f64) = body b of the handle; ordered against caller_stream exactly as tetsim_observe_bodies_device */
int tetsim_body_poses_device(tetsim_handle h, void *dst, uint64_t row_stride, void *caller_stream);
/* the same rows into host memory [num_bodies * TETSIM_POSE_WIDTH]; synchronises */
int tetsim_read_body_poses(tetsim_handle h, double *out);
/* Host only, no device: the constant per-particle table those calls build, records_out[nv * 32 bytes] = { double m, qx, qy, qz }, and
 * per body { double c0[3] } into centres_out[3 * num_bodies] (may be NULL).  body_first_vert / body_first_tet: [num_bodies + 1] as
 * tetsim_create_batch lays them out; both NULL = one body (num_bodies is then taken as 1). */
int tetsim_prep_pose_table(const float *verts, uint32_t nv, const int32_t *tets, uint32_t nt,
                           const uint32_t *body_first_vert, const uint32_t *body_first_tet, uint32_t num_bodies,
                           double density, void *records_out, double *centres_out);

/* --- touch sensing on the device: per-body contacts with the colliders ------------------------- */

/* Whether a body rests on its tray, is pinched by a jaw or has slipped off a paddle: the contacts of every body with the colliders
 * ITS substeps meet -- per body and collider slot the touching particles, the least distance, the centroid, the mean normal and the mean
 * relative velocity (tetsim_touch_bodies_device; tetsim_read_body_touch on the host), or per particle the nearest collider
 * (tetsim_touch_particles_device: a tactile skin, a channel to colour by).  A read-only, GEOMETRIC query of the stored state: no solver
 * state changes, no stepping kernel knows of it, held particles are included, and nothing is recorded inside a substep.  An ADDITIVE
 * extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look the symbols up.
 *
 * THE LIST of a body is the one its substeps walk: while body colliders are ON (tetsim_set_body_colliders) the body's compacted table
 * entries -- slot k is its k-th non-empty row -- otherwise the handle's list (tetsim_set_colliders), slot k = collider k.  Its values are
 * the ones the substeps read -- the f32 view of a POLAR_JACOBI or FAST NEOHOOKEAN_GS handle, the f64 view of a PRECISE NEOHOOKEAN_GS
 * handle, normalised as described there -- widened to f64.
 *
 * DEFINITIONS.  p = a stored f32 position widened to f64 (what tetsim_read_positions returns).  All arithmetic is f64, every operation
 * rounded on its own (no fused multiply-add), / and sqrt correctly rounded; dot(u,v) = (u.x*v.x + u.y*v.y) + u.z*v.z.  The signed
 * distance sd and the outward unit normal n of p against one collider continue the hit test of tetsim_set_colliders to the outside:
 *   sphere   d = p - a, L = sqrt(dot(d, d)); sd = L - radius; n = d / L if L > 0, else n = 0
 *   capsule  ab = b - a, t = dot(p - a, ab) / dot(ab, ab) (0 if dot(ab, ab) == 0), t = min(max(t, 0), 1); d = p - (a + ab*t), as the sphere
 *   plane    sd = dot(p - a, b); n = b
 *   box      l_k = dot(p - a, u_k), g_k = e_k - |l_k| (e = b, the half-extents).  If g_k >= 0 for every k (inside or on the box):
 *            k = argmin g_k (lowest k on ties), sd = -g_k, n = l_k >= 0 ? u_k : -u_k.  Otherwise o_k = max(-g_k, 0) (NaN for a NaN g_k),
 *            sd = sqrt((o_0*o_0 + o_1*o_1) + o_2*o_2), w = the sum over k = 0, 1, 2 of (l_k >= 0 ? o_k : -o_k) * u_k, added component by
 *            component from 0.0, n = w / sd.
 * WHERE THE STEP WOULD PUSH: wherever the f64 hit test of tetsim_set_colliders hits p, sd < 0, -sd is bit for bit the depth and n bit for
 * bit the normal of that push.  (A particle at rest on a collider was pushed OUT by its last substep and stored in f32, so it sits within
 * a few f32 roundings of sd = 0, on either side (measured: -1e-7 .. 0): that is what `margin` is for.)
 * A particle TOUCHES a slot when sd < margin (metres; any finite value, negative ones too).  A NaN sd never touches and is never a
 * minimum; minima are taken over ALL particles of the body, touching or not (the distance still to go), by fmin.
 *
 * THE BODY ROW, TETSIM_TOUCH_WIDTH doubles:
 *   [0] TOUCHING  particles that touch at least one slot          [1] MIN_SD    the least sd over all slots and particles, +inf if none
 *   [2] MIN_SLOT  the first slot whose MIN_SD is below every      [3] SLOTS     the length of the body's list
 *                 earlier one's (ascending scan with <), or -1
 *   [4 + 12k ..] slot k, TETSIM_TOUCH_SLOT_WIDTH doubles:
 *   [0] KIND      0..3                [1] COUNT   touching particles         [2] MIN_SD   the slot's least sd, +inf if none
 *   [3..5] CENTROID = (S p) / COUNT   [6..8] NORMAL = (S n) / COUNT          [9..11] REL_VEL = (S (v - V)) / COUNT
 *   S: the sum over the slot's touching particles, v the stored f32 velocity widened, V the collider's velocity; COUNT == 0 gives nine
 *   zeros.  A slot k >= SLOTS reads KIND -1, MIN_SD +inf and ten zeros.  Counts are reduced as integers and stored as doubles.
 * REPRODUCIBLE AND POSITION INDEPENDENT, as the observation: a body's particles are cut into chunks of 256 counted from its own first
 * particle, a chunk is reduced by the fixed tree, the chunks' rows are folded in index order by the same tree; particles that do not
 * touch contribute 0.0 to the sums; no atomics.  Two calls give the same bits, a body of a batch the bits it gives alone with
 * tetsim_set_colliders of the same rows.
 * THE PARTICLE ROW, TETSIM_TOUCH_PARTICLE_WIDTH f32 for each of the handle's particles in the caller's numbering, every value the f64
 * result rounded once:
 *   [0] sd of the nearest slot (ascending scan with <: ties go to the lower slot; +inf without a slot or with NaN everywhere)
 *   [1..3] that slot's n (0 without one)      [4] the slot as a value, or -1      [5] the number of slots the particle touches      [6..7] 0
 *
 * Body rows: row b of dst = body b (tetsim_get_batch_layout) at dst + b * row_stride, 8-byte aligned, the stride 0 (packed: 800) or a
 * multiple of 8 of at least 800.  Particle rows: row i at dst + i * row_stride, 4-byte aligned, the stride 0 (packed: 32) or a multiple
 * of 4 of at least 32.  Only the rows' own values are written -- not the padding of a wider row, not a byte outside the rows.  THE
 * STREAM CONTRACT is that of tetsim_observe_bodies_device: the handle's stream waits for caller_stream, the launches (two for the
 * body rows, one for the particle rows) run behind every substep and every set call enqueued so far, caller_stream waits for them.
 * Only the handle's first touch call may block: it allocates the scratch of the chunk rows (90 doubles per chunk of 256 particles)
 * and the rows of the host read and, unless another per-body call made it, uploads the handle's particle chunk table; all of it
 * counts into TetSimInfo.device_bytes from then on.  tetsim_read_body_touch writes the body rows to host memory,
 * out[num_bodies * TETSIM_TOUCH_WIDTH], and synchronises.  A handle without colliders is legal: SLOTS 0, MIN_SD +inf, MIN_SLOT -1,
 * every particle's slot -1.
 * THE KERNELS.  One workgroup per chunk of 256 particles, which belong to one body: its list arrives by scalar loads (the handle's
 * list travels as a kernel argument), a lane holds one particle and walks the slots, ten f64 accumulators and a count per slot go
 * through the tree and leave through the first lane; one workgroup per body folds the chunk rows slot by slot and its first lane
 * divides.  No scratch memory (94 / 112 / 72 VGPRs for the chunk, finish and particle kernels).  Cost, measured on an MI355X against the
 * observation on the same batch in the same run (tools/touch_cost.py, profiles/touch_cost.txt): 64 Dragons (78,976
 * particles) in one batch, per call, the observation 41.5 us; the body rows 32.5 us with no slot (x0.78), 56.1 us with four slots per
 * body (x1.35), 79.2 us with eight (x1.91) -- about 6 us per slot; the particle rows 28.2, 30.1 and 33.1 us (x0.68, x0.72, x0.80).
 *
 * Every error is found before anything is enqueued and leaves `dst` as it was.  TETSIM_EINVAL: a NULL handle, dst or out; a margin
 * that is not finite; a dst that is not aligned as above; such a row_stride; a dst that hipPointerGetAttributes does not report as
 * device memory of the handle's device, or whose rows do not fit the allocation it points into.  TETSIM_ESTATE: a partitioned body.
 * Out of scope: contact forces or impulses recorded inside the substep; contacts between bodies; per-body margins; a body mask;
 * partitioned bodies; a Node binding; gradients. */
#define TETSIM_TOUCH_WIDTH 100           /* doubles per body row: 800 bytes */
#define TETSIM_TOUCH_SLOT_WIDTH 12       /* doubles per slot of a body row */
#define TETSIM_TOUCH_PARTICLE_WIDTH 8    /* floats per particle row: 32 bytes */
enum { TETSIM_TOUCH_TOUCHING = 0, TETSIM_TOUCH_MIN_SD = 1, TETSIM_TOUCH_MIN_SLOT = 2, TETSIM_TOUCH_SLOTS = 3,
       TETSIM_TOUCH_SLOT0 = 4 /* slot k at SLOT0 + k * TETSIM_TOUCH_SLOT_WIDTH */ };
enum { TETSIM_TOUCH_SLOT_KIND = 0, TETSIM_TOUCH_SLOT_COUNT = 1, TETSIM_TOUCH_SLOT_MIN_SD = 2, TETSIM_TOUCH_SLOT_CENTROID = 3 /*..5*/,
       TETSIM_TOUCH_SLOT_NORMAL = 6 /*..8*/, TETSIM_TOUCH_SLOT_REL_VEL = 9 /*..11*/ };
enum { TETSIM_TOUCH_P_SD = 0, TETSIM_TOUCH_P_NORMAL = 1 /*..3*/, TETSIM_TOUCH_P_SLOT = 4, TETSIM_TOUCH_P_TOUCHES = 5,
       TETSIM_TOUCH_P_RESERVED = 6 /*..7, written as 0*/ };
/* row b of dst (DEVICE memory, f64) = body b of the handle; ordered against caller_stream exactly as tetsim_observe_bodies_device */
int tetsim_touch_bodies_device(tetsim_handle h, double margin, void *dst, uint64_t row_stride, void *caller_stream);
/* the same rows into host memory [num_bodies * TETSIM_TOUCH_WIDTH]; synchronises */
int tetsim_read_body_touch(tetsim_handle h, double margin, double *out);
/* row i of dst (DEVICE memory, f32) = particle i of the caller's numbering; ordered against caller_stream likewise */
int tetsim_touch_particles_device(tetsim_handle h, double margin, void *dst, uint64_t row_stride, void *caller_stream);

/* --- range sensors on the device: per-body ray casts from device memory ------------------------- */

/* What a depth or touch sensor attached to ONE body of a batch needs: rays, the body each ray belongs to and the hits live in the
 * caller's DEVICE memory, nothing synchronises the host, and a ray is cast against ITS OWN body -- the bodies of a batch usually
 * occupy the same region of space, where tetsim_raycast_visual would answer "body 0" for every ray.  An ADDITIVE extension of ABI
 * version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look the symbols up.
 *
 * DEFINITIONS.  rays: count TetSimRay records, record i at rays + i * ray_stride; hits: count TetSimRayHit records at
 * hits + i * hit_stride; ray_body: count int32, packed, or NULL.  The arithmetic is that of tetsim_raycast_visual (above), bit for bit.
 *   ray_body == NULL: record i is exactly what tetsim_raycast_visual returns for ray i, in every field, `body` included.
 *   ray_body != NULL: ray i is cast against body b = ray_body[i] alone: it sees the triangles whose rows belong to b, in the order of the
 *     caller's list, and is culled by the bounding sphere of b's visual rows.  The record is what tetsim_raycast_visual returns for body
 *     b created ALONE in the same state, bit for bit, except that `triangle` is the position in THIS handle's list and body = b.  A
 *     single body accepts ray_body values of 0.  A body without visual rows or without triangles gives a miss.
 *   An invalid ray cannot be refused by the host, which never sees it: the device gives it hit = TETSIM_RAY_INVALID, body = triangle =
 *     -1 and zeros elsewhere, and it disturbs no other ray.  Invalid is what tetsim_raycast_visual refuses -- a non-finite origin or
 *     direction, a zero direction, a NaN near or far, near < 0, far < near -- and a ray_body value outside [0, num_bodies).
 * tetsim_visual_bounding_spheres_device: row b of dst = (centre x, y, z, radius) of body b's visual rows, 4 doubles at
 * dst + b * row_stride: what tetsim_read_visual_bounding_sphere returns for body b alone, bit for bit (the same order-free reduction
 * on integer keys, one set per body; "bit for bit" holds for finite positions: a NaN component is left out of the box, and which other
 * rows that takes with it depends, here as in tetsim_read_visual_bounding_sphere, on how the rows fall into waves).  A body without rows
 * gives (0, 0, 0, 0), as three.js does for an empty Box3.
 * Only the 48 bytes of a hit record and the 32 bytes of a sphere row are written: not the padding of a wider row, not a byte outside.
 *
 * THE KERNEL.  One lane per ray, 256 rays per workgroup; a body's triangles pass through the workgroup's LDS in tiles of 256, each
 * prepared once (gathered, converted to f64, edges and normal) and then read by every ray of that body.  RAYS GROUPED BY BODY ARE THE
 * FAST CASE: a workgroup whose rays name several bodies goes through those bodies one after the other (the answers do not depend on
 * the grouping).  Few rays split the triangle range over more workgroups; the winner is the smallest (distance, triangle) in
 * lexicographic order at every level, so it depends on no grid shape.  Any count works.
 *
 * THE STREAM CONTRACT is that of tetsim_export_device: the handle's stream waits for an event on caller_stream (rays and bodies are
 * then complete, hits / dst free), the work -- skinning first, as every query, so the answer belongs to the last substep enqueued
 * before the call -- runs behind every substep enqueued so far, caller_stream waits for it.  No host synchronisation, and no solver
 * state changes.  Only a handle's first such call may block: it builds the per-body tables on the host (per row its body, the triangle
 * ids stably sorted by body with the bodies' offsets, per triangle its body) and uploads them with a scratch buffer whose size does
 * not depend on count; all of it counts into TetSimInfo.device_bytes from then on.
 *
 * Every error is found before anything is enqueued and leaves hits / dst as they were.  TETSIM_EINVAL: a NULL handle; NULL rays or
 * hits with count > 0; a NULL dst; a stride that is neither 0 (packed: 64 / 48 / 32) nor a multiple of 8 of at least that; a pointer
 * that is not 8-byte aligned (ray_body: 4-byte), that hipPointerGetAttributes does not report as device memory of the handle's
 * device, or whose rows do not fit the allocation it points into.  TETSIM_ESTATE: no visual mesh; no triangles (the ray call only); a
 * partitioned body; with ray_body != NULL a triangle whose three rows belong to different bodies (found once on the host; such a
 * mesh still casts with ray_body == NULL).  count == 0 succeeds and enqueues nothing.
 * Out of scope: partitioned bodies; an acceleration structure behind THIS call (tetsim_raycast_visual_bvh_device below is the same
 * call through one); all hits along a ray; back-side or double-side materials; f32 rays or
 * hits; rays attached to a moving frame (the caller transforms them, on the device, before the call); gradients; a Node
 * binding (Node has no device tensors). */
#define TETSIM_RAY_INVALID (-1)   /* TetSimRayHit.hit of a ray the device refused */
int tetsim_raycast_visual_device(tetsim_handle h,
        const void *rays,     uint64_t ray_stride,   /* DEVICE: count TetSimRay records (64 B); stride 0 = packed, else a multiple of 8, >= 64 */
        const void *ray_body,                        /* DEVICE: count int32, or NULL */
        uint32_t count,
        void *hits,           uint64_t hit_stride,   /* DEVICE: count TetSimRayHit records (48 B); stride 0 = packed, else a multiple of 8, >= 48 */
        void *caller_stream);
/* one row of 4 doubles per body (centre xyz, radius) into DEVICE memory; stride 0 = packed 32, else a multiple of 8, >= 32 */
int tetsim_visual_bounding_spheres_device(tetsim_handle h, void *dst, uint64_t row_stride, void *caller_stream);

/* --- range sensors through a refitted bounding-volume hierarchy --------------------------------- */

/* tetsim_raycast_visual_device is brute force, every ray against every triangle of its body: a 32 x 32 depth image of a Dragon costs
 * a hundred frames of its physics.  tetsim_raycast_visual_bvh_device is its twin -- the signature, the records, the stream contract and
 * the list of errors are those of tetsim_raycast_visual_device, word for word -- and answers from a tree of boxes per body that is
 * refitted on the device at every call.  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct
 * changed): look the symbol up.
 *
 * THE DEFINITION is its own, and it does not mention the tree: a culling structure cannot promise three.js's answer for a ray that lies
 * nearly in a triangle's plane, where step 3 of tetsim_raycast_visual may accept a "hit" whose computed point lies anywhere.  So the
 * call is defined as brute force with two more conditions per triangle, stated so that ANY conservative tree reproduces it bit for bit;
 * it differs from tetsim_raycast_visual_device only for hits that are numerically meaningless (tests/raycast_bvh_ref.py is the
 * definition in numpy).  f64, every operation rounded separately.
 *   Steps 1 and 2 of tetsim_raycast_visual -- the sphere cull and the normalised direction d -- as they are, with the sphere of the
 *   ray's body (ray_body == NULL: of the whole mesh); o = origin.
 *   Padding:  e = 2^-20 * (radius + sqrt(dot(o - centre, o - centre))), centre and radius of that sphere.
 *   Padded box of a triangle with f32 corners: lo_k / hi_k = the smallest / largest of the three corners' component k (exact, taken as
 *     doubles); L_k = lo_k - e, H_k = hi_k + e.
 *   Slab interval: tn = -inf, tf = +inf; for k = 0, 1, 2:  inv = 1.0 / d_k;  if d_k == 0 or inv is infinite, axis k passes iff
 *     L_k <= o_k && o_k <= H_k, and leaves tn, tf alone;  else t1 = (L_k - o_k) * inv, t2 = (H_k - o_k) * inv,
 *     tn = max(tn, min(t1, t2)), tf = min(tf, max(t1, t2)).
 *   The triangle is a CANDIDATE iff every axis passes and tn <= tf.  A candidate COUNTS iff step 3 of tetsim_raycast_visual accepts it,
 *     the near / far window included, and tn <= distance && distance <= tf.
 *   The record is the smallest (distance, triangle) among the counting hits, in lexicographic order; point and distance are step 3's for
 *     that triangle.  Invalid rays, misses, `body` and `triangle` are those of tetsim_raycast_visual_device.
 * Why a tree reproduces this: every comparison above is false for a NaN (none arises from finite inputs), and the operations are monotone
 * in IEEE arithmetic -- a node's f32 box that contains a triangle's box has tn <= the triangle's tn, tf >= its tf, and its axis tests
 * pass wherever the triangle's do.  The traversal skips a node only if its own test (same formulas, same e) fails, tn > far, tf < near,
 * or a best hit exists and tn > its distance (tn == best is entered: a lower triangle index may tie); at a leaf every triangle gets the
 * box of its OWN corners.  Visit order and tree shape then cannot change a bit of the answer.
 *
 * THE TREE.  Topology: built once per handle by its first such call, on the host, from the skinned positions of that moment -- per body
 * the triangles of its own surface in the Morton order of their centroids, four to a leaf, under a complete binary tree in heap order
 * (no pointers; a body without triangles or with one is a tree of one leaf).  That call may block and synchronise once, like the first
 * tetsim_raycast_visual_device call, whose tables it extends; what it allocates counts into TetSimInfo.device_bytes from then on and does
 * not depend on count.  The topology never changes: a body deformed beyond recognition is answered as exactly, only more slowly.
 * Refit: at EVERY call, on the handle's stream behind the skinning -- exact f32 min / max, leaves from corners, nodes from children,
 * all bodies together in two launches whatever their number; no host synchronisation.  Traversal: one lane per ray, near child first,
 * stackless.  With ray_body == NULL a ray walks the bodies' trees, lowest body first, carrying its best; a triangle whose rows span bodies
 * then belongs to the body of its first row.  Rays need NOT be grouped by body: a workgroup's rays may name any mix of bodies.
 * When to use which: INTEGRATION.md 4f.  Out of scope: this structure behind the host calls; rebuilding the topology; and what
 * tetsim_raycast_visual_device leaves out. */
int tetsim_raycast_visual_bvh_device(tetsim_handle h,
        const void *rays,     uint64_t ray_stride,   /* as tetsim_raycast_visual_device */
        const void *ray_body,
        uint32_t count,
        void *hits,           uint64_t hit_stride,
        void *caller_stream);

/* --- closest-point queries through the refitted tree -------------------------------------------- */

/* How far is this point from that body's surface, and where on the surface is the nearest point: what a distance reward, a proximity
 * sensor, a marker fixed to the surface and contact generation for another engine ask.  Queries, the body each belongs to and the
 * records live in the caller's DEVICE memory, nothing synchronises the host, and a query is answered by ITS OWN body through the tree
 * of tetsim_raycast_visual_bvh_device.  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct
 * changed): look the symbols up.  The stream contract, the pointer, stride and allocation checks, "every error is found before anything
 * is enqueued and leaves `out` as it was", "count == 0 succeeds" and the TETSIM_ESTATE cases are those of
 * tetsim_raycast_visual_bvh_device, word for word, with queries / query_body / out in the places of rays / ray_body / hits (strides:
 * 0 = packed 32 / 64, else a multiple of 8 of at least that).  Only the 64 bytes of a record are written.
 *
 * THE DEFINITION is brute force and does not mention the tree (tests/closest_ref.py is the definition in numpy).  f64, every operation
 * rounded separately, sums left to right.  queries: count TetSimPointQuery records; query_body: count int32, packed, or NULL.
 *   A query is INVALID if a component of its point is not finite, its max_distance is NaN or < 0 (+infinity is allowed), or its
 *     query_body value is outside [0, num_bodies): found = TETSIM_CLOSEST_INVALID, body = triangle = region = -1 and zeros elsewhere.
 *     It disturbs no other query.  (The host variant sees its queries and refuses such a one with TETSIM_EINVAL.)
 *   The triangles: with query_body, those whose rows belong to body b = query_body[i], and the bounding sphere of b's visual rows; without,
 *     all of them and the sphere of the whole mesh -- the spheres of the ray casts.  A single body accepts query_body values of 0.
 *   Per triangle (a, b, c: the f32 corners taken as doubles; p: the point) the closest point q is three.js r160
 *     Triangle.closestPointToPoint, in the order of its operations:  ab = b - a, ac = c - a, ap = p - a, d1 = ab.ap, d2 = ac.ap;
 *     d1 <= 0 && d2 <= 0: q = a.  bp = p - b, d3 = ab.bp, d4 = ac.bp;  d3 >= 0 && d4 <= d3: q = b.  vc = d1*d4 - d3*d2;
 *     vc <= 0 && d1 >= 0 && d3 <= 0: v = d1 / (d1 - d3), q = a + ab*v.  cp = p - c, d5 = ab.cp, d6 = ac.cp;  d6 >= 0 && d5 <= d6: q = c.
 *     vb = d5*d2 - d1*d6;  vb <= 0 && d2 >= 0 && d6 <= 0: w = d2 / (d2 - d6), q = a + ac*w.  va = d3*d6 - d5*d4;
 *     va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), q = b + (c - b)*w.  Otherwise
 *     denom = 1 / ((va + vb) + vc), v = vb*denom, w = vc*denom, q = (a + ab*v) + ac*w.  (x.y = x0*y0 + x1*y1 + x2*y2.)
 *   region and (v, w), with q = a + v*ab + w*ac in exact terms:  1 vertex a (0, 0);  2 vertex b (1, 0);  3 vertex c (0, 1);  4 edge ab
 *     (v, 0);  5 edge ac (0, w);  6 edge bc (1.0 - w, w), w the method's;  0 the face (v, w).
 *   d2 = dot(p - q, p - q).
 *   Padding:  e = 2^-20 * (radius + sqrt(dot(p - centre, p - centre))), centre and radius of the sphere above.
 *   Box bound of a triangle:  lo_k / hi_k = the smallest / largest of the three corners' component k;  L_k = lo_k - e, H_k = hi_k + e;
 *     g_k = the largest of L_k - p_k, p_k - H_k and 0;  lb = g_0*g_0 + g_1*g_1 + g_2*g_2.
 *   A triangle COUNTS iff lb <= d2 && d2 <= max_distance * max_distance.  (A zero-area triangle whose q is NaN never counts.)
 *   The record is the smallest (d2, triangle) among the counting triangles, in lexicographic order: found = 1, distance = sqrt(d2);
 *     point, region, v, w are that triangle's; triangle is the position in THIS handle's list; body is the query's body, or without
 *     query_body the body of the triangle's first row.  When none counts: found = 0, body = triangle = region = -1, zeros elsewhere.
 * Why a tree reproduces this bit for bit: every comparison above is false for a NaN, and lb is monotone in the box in IEEE arithmetic -- a
 * node's f32 box that contains a triangle's box has lb_node <= lb_triangle (same formulas, same e).  The traversal skips a node only if
 * it is empty, lb_node > max_distance^2, or a best exists and lb_node > d2_best -- strictly: a node with lb_node == d2_best is entered,
 * because a lower triangle index may tie.  At a leaf every triangle is tested with the box of its OWN corners.  The running best is
 * never below the winner's d2 and the winner counts (lb <= d2), so no ancestor of the winner is skipped, whatever the visit order and
 * the tree's shape.  (lb <= d2 holds for every triangle in exact arithmetic -- q lies in the triangle's box --, and e dwarfs the
 * rounding: the predicate removes nothing, tests/test_closest_cpu.py counts 0; it is there so that the argument needs no error analysis.)
 *
 * THE TREE is that of tetsim_raycast_visual_bvh_device: built once per handle by its first tree call -- ray cast or closest point,
 * whichever comes first; only that call may block --, refitted at EVERY call on the handle's stream behind the skinning and the spheres.
 * What the first call allocates counts into TetSimInfo.device_bytes from then on and does not depend on count.  THE KERNEL: one lane per
 * query, 256 per workgroup, stackless as the ray cast's; both children's boxes in one 48-byte read, the child with the smaller bound
 * first; the lanes of a wave reach their leaves together before a leaf's four triangles are gathered and tested.  With query_body ==
 * NULL a lane walks the bodies' trees, lowest body first, carrying its best.  Queries need not be grouped by body.  No scratch memory,
 * 138 VGPRs (three waves a SIMD, as the ray cast).  Cost, measured on an MI355X beside the ray cast through the same tree in the same run
 * (tools/closest_cost.py, profiles/closest_cost.txt): 64 Dragons (59,657 triangles each) in one batch, 65,536 queries
 * scattered within one bounding radius of their bodies' surfaces and shuffled over the bodies, 4.05 ms per call against 1.95 ms for
 * as many rays (x2.08); the refit is 0.18 ms of it (4.4 %); a query tests 365 boxes and 185 triangles on average.
 *
 * tetsim_closest_visual: the same records for host arrays -- staged through buffers that grow on demand, the same kernel, one
 * synchronisation.  TETSIM_EINVAL for a query the device variant would mark invalid (the message names the first).
 * Out of scope: an inside / outside sign (it needs pseudo-normals; `region` tells the caller when the face normal can be trusted: 0);
 * the k nearest; queries against the tet mesh itself; a Node binding; partitioned bodies; gradients. */
typedef struct TetSimPointQuery { double point[3], max_distance; } TetSimPointQuery;          /* 32 B; max_distance may be +inf */
typedef struct TetSimClosest    { int32_t found, body, triangle, region;
                                  double distance, point[3], v, w; } TetSimClosest;           /* 64 B */
#define TETSIM_CLOSEST_INVALID (-1)   /* TetSimClosest.found of a query the device refused */
int tetsim_closest_visual_device(tetsim_handle h,
        const void *queries,  uint64_t query_stride,   /* DEVICE; stride 0 = packed 32, else a multiple of 8, >= 32 */
        const void *query_body,                        /* DEVICE: count int32, or NULL */
        uint32_t count,
        void *out,            uint64_t out_stride,     /* DEVICE; stride 0 = packed 64, else a multiple of 8, >= 64 */
        void *caller_stream);
int tetsim_closest_visual(tetsim_handle h, const TetSimPointQuery *queries, const int32_t *query_body, uint32_t count, TetSimClosest *out);  /* host arrays; synchronises */

/* --- per-tet strain on the device: deformation gradient, volume ratio, principal stretches ------ */

/* How deformed the material is: per tet the deformation gradient the reference's solveElem computes and throws away (Softbody.js:103-109,
 * 159), its determinant, the principal stretches and a scalar strain to colour a mesh by; per body how far it is stretched and whether it
 * has been crushed; per visual vertex one of those values.  All of it in the caller's DEVICE memory, with no host synchronisation, from the
 * library's own invRestPose.  An ADDITIVE extension of ABI version 5 (TETSIM_ABI_VERSION is unchanged; no existing struct changed): look
 * the symbols up.
 *
 * DEFINITIONS.  All arithmetic is f64 on the stored f32 values -- the positions tetsim_read_positions returns and the f32 invRestPose B
 * tetsim_prep_rest returns (column-major: B_ij = inv_rest_pose[9 * tet + 3 * j + i]) --, every operation rounded on its own (no fused
 * multiply-add), sums left to right as written, and only + - * / sqrt, so that tests/strain_ref.py gives the same bits in numpy.  Per tet
 * with corners 0..3 in the caller's numbering (a batch: the concatenation), x_k the current positions:
 *   P       column k = x_(k+1) - x_0:  P_ik = x_(k+1)[i] - x_0[i]
 *   F       = P * B:  F_ij = (P_i0*B_0j + P_i1*B_1j) + P_i2*B_2j                             (9 floats, column-major: F_ij at F + 3 * j + i)
 *   J       = (F00*(F11*F22 - F12*F21) - F01*(F10*F22 - F12*F20)) + F02*(F10*F21 - F11*F20)
 *   C       = F^T F, each pair once:  C_ij = (F0i*F0j + F1i*F1j) + F2i*F2j   (i <= j)
 *   DEV     = sqrt((C00 + C11) + C22)                                                          the reference's r_s; sqrt 3 at rest
 *   GREEN   = the Frobenius norm of E = (C - I) / 2:  E_ii = (C_ii - 1) / 2, E_ij = C_ij / 2, and
 *             GREEN = sqrt(((((E00*E00 + E11*E11) + E22*E22) + 2*(E01*E01)) + 2*(E02*E02)) + 2*(E12*E12))      0 for any rigid motion
 *   STRETCH = sqrt(e < 0 ? 0 : e) of the three diagonal entries e of C after the Jacobi procedure below, then put in DESCENDING order by
 *             three compare-and-swaps (0,1), (0,2), (1,2) that swap where the earlier value is smaller (3 floats)
 * Values are rounded to f32 once, at the store.  RESERVED is written as 0.
 * A DEGENERATE tet -- its rest volume (the observation's V0, above) is 0, or its invRestPose holds a non-finite value; found once on the
 * host -- gives NaN in 0..14.
 *
 * THE JACOBI PROCEDURE.  TETSIM_STRAIN_SWEEPS cyclic sweeps over the pairs (0,1), (0,2), (1,2), no convergence test: a NaN terminates
 * and every lane does the same work.  For a pair (p,q), r the third index:  nothing if C_pq == 0;  otherwise
 *   theta = (C_qq - C_pp) / (2*C_pq)      t = sgn(theta) / (|theta| + sqrt(theta*theta + 1)), sgn(0) = +1
 *   c = 1 / sqrt(t*t + 1)                 s = t*c
 *   C_pp -= t*C_pq     C_qq += t*C_pq     (C_rp, C_rq) <- (c*C_rp - s*C_rq, s*C_rp + c*C_rq)     C_pq = 0
 * WHY 4 SWEEPS.  It is the smallest count at which tests/strain_ref.py agrees with numpy.linalg.svd on the inputs of
 * tests/test_strain_cpu.py (4,000 seeded F with condition numbers up to 1e6, near-equal pairs, rank 1 and 2, J < 0; the stepped Dragon
 * states of tests/golden) within that test's margin: with d = (24 * sweeps + 8) * 2^-53 * trace(C) for the eigenvalues, a stretch is
 * within min(d / sigma, sqrt(d)) + 4 * 2^-53 * sigma_max of LAPACK's sigma.  Observed at 4 sweeps: 0.11 of that margin at worst (3 sweeps:
 * 22 times the margin on the seeded set, 1,000 times on a Dragon state), the off-diagonal entries left behind below 3e-7 * 2^-53 *
 * trace(C), and the largest |stretch - sigma| / sigma_max = 1.2e-8, on a rank-2 F, where a square root of a rounding error is all any
 * method through C can give.
 *
 * THE BODY ROW (tetsim_body_strain_device): TETSIM_STRAIN_BODY_WIDTH doubles per body of the handle, reduced from the f64 values before
 * they are rounded to f32:  [0] the largest stretch, [1] the smallest stretch, [2] min J, [3] max J, [4] max GREEN,
 * [5] the sum of |V0| * (GREEN*GREEN), [6] the sum of |V0|, [7] the number of tets LEFT OUT of all of these: the degenerate ones and
 * those with a non-finite value in 0..14 of their f32 row (a count, reduced as an integer and stored as a double).  A body without usable
 * tets reports -inf, +inf, +inf, -inf, -inf, 0, 0, n.  The reduction is the observation's: chunks of 256 tets counted from the body's own
 * first tet, a fixed tree inside a chunk, the chunks' partial rows in index order by the same tree, no floating-point atomics -- a body of
 * a batch gives the bits it gives alone, and two calls give the same bits.  The per-tet rows are not materialised.
 *
 * VISUAL STRAIN (tetsim_visual_strain_device): one float per attached visual row at dst + row * row_stride: channel `channel` (0..14) of
 * the tet visVerts[row].tetNr, bit for bit the value of that tet's row.
 *
 * Row t of dst = tet t in the caller's numbering at dst + t * row_stride (row b = body b for the body row); only the payload of a row is
 * written -- not the padding of a wider row, not a byte outside the rows.  THE STREAM CONTRACT is that of tetsim_export_device: the
 * handle's stream waits for caller_stream, the work runs behind every substep enqueued so far, caller_stream waits for it; no host
 * synchronisation.  Only a handle's first strain call may block: it builds the constant per-tet table on the host (64 bytes per tet: the
 * four particle ids, the nine f32 of invRestPose, the degenerate mark, |V0|) and uploads it with the scratch of the partial rows and the
 * rows of the host read (the first visual call: the rows' tets) and, unless an observation made it, the handle's tet chunk table (the
 * observation's); all of it counts into TetSimInfo.device_bytes from then on.
 * tetsim_read_tet_strain writes the tet rows to host memory, out[num_elems * TETSIM_STRAIN_WIDTH], and synchronises.
 * THE KERNEL.  One lane per tet, 256 per workgroup; a lane reads its record as four 16-byte loads and gathers four corners.  Packed rows
 * (row_stride 64) at a 16-byte aligned dst pass through LDS and leave as 16-byte stores that cover contiguous memory wave by wave;
 * anything else leaves as dword stores per row.  The same bits either way.
 *
 * Every error is found before anything is enqueued and leaves `dst` as it was.  TETSIM_EINVAL: a NULL handle, dst or out; a dst that is
 * not 4-byte aligned (body row: 8-byte); a row_stride that is neither 0 (packed: 64; visual: 4) nor a multiple of 4 (body row: 8) of at
 * least the row's bytes; a dst that hipPointerGetAttributes does not report as device memory of the handle's device, or whose rows do not
 * fit the allocation it points into; a channel outside 0..14.  TETSIM_ESTATE: a partitioned body; tetsim_visual_strain_device without a
 * visual mesh.  A handle with 0 tets succeeds: no tet rows are written (the body row reports "no usable tets").
 * Out of scope: partitioned bodies; a Node binding; energies that need compliances; stress; gradients; a body mask. */
#define TETSIM_STRAIN_WIDTH 16        /* floats per tet row: 64 bytes */
#define TETSIM_STRAIN_BODY_WIDTH 8    /* doubles per body row: 64 bytes */
#define TETSIM_STRAIN_SWEEPS 4        /* cyclic Jacobi sweeps behind STRETCH */
enum { TETSIM_STRAIN_F = 0 /*..8, column-major*/, TETSIM_STRAIN_J = 9, TETSIM_STRAIN_DEV = 10,
       TETSIM_STRAIN_STRETCH = 11 /*..13, descending*/, TETSIM_STRAIN_GREEN = 14, TETSIM_STRAIN_RESERVED = 15 /* written as 0 */ };
/* row t of dst (DEVICE memory, f32) = tet t in the caller's numbering; ordered against caller_stream exactly as tetsim_export_device */
int tetsim_tet_strain_device(tetsim_handle h, void *dst, uint64_t row_stride, void *caller_stream);
/* the same rows into host memory [num_elems * TETSIM_STRAIN_WIDTH]; synchronises */
int tetsim_read_tet_strain(tetsim_handle h, float *out);
/* row b of dst (DEVICE memory, f64) = body b of the handle */
int tetsim_body_strain_device(tetsim_handle h, void *dst, uint64_t row_stride, void *caller_stream);
/* one float per attached visual row (DEVICE memory): channel `channel` of the row's tet */
int tetsim_visual_strain_device(tetsim_handle h, int32_t channel, void *dst, uint64_t row_stride, void *caller_stream);
/* Host only, no device: the constant per-tet table those calls build, records_out[nt * 64 bytes].  A record is { int32 ids[4]; float
 * inv_rest_pose[9] (what tetsim_prep_rest returns for the tet); uint32 degenerate (0 / 1); double abs_v0 }. */
int tetsim_prep_strain_table(const float *verts, uint32_t nv, const int32_t *tets, uint32_t nt, double density, void *records_out);

/* --- measurement ----------------------------------------------------------------------------- */

/* Run n substeps eagerly on the handle's own stream; every POLAR_JACOBI kernel carries its own begin/end HIP
 * events (hipExtLaunchKernelGGL), so kernel_ms[] sums the kernels' own durations in the real launch sequence.  Bodies with
 * TetSimInfo.fused_particle_pass run the sequence of tetsim_step_n (tet | fused x (n-1) | particle): TETSIM_K_TET then holds the
 * n-1 fused kernels, TETSIM_K_VERTEX the one particle kernel that ends the call. */
int tetsim_profile(tetsim_handle h, uint32_t n, double dt, const TetSimParams *params, TetSimProfile *out);
/* Kernel-only timing: `reps` back-to-back launches of the per-tet kernel(s) of one substep inside ONE HIP-event
 * pair on the handle's stream, then the same for the per-particle kernel(s); kernel_ms[] = total / reps.  No event
 * sits between kernels, so the figure is comparable with rocprofv3's per-kernel average.  The body is left in a
 * finite but NON-PHYSICAL state (kernels are repeated out of sequence): call it on a scratch body. */
int tetsim_time_kernels(tetsim_handle h, uint32_t reps, double dt, const TetSimParams *params, TetSimProfile *out);
/* n substeps through the production path (tetsim_step_n), bracketed by HIP events on the handle's
 * stream; returns elapsed milliseconds.  Synchronises. */
int tetsim_time_step_n(tetsim_handle h, uint32_t n, double dt, const TetSimParams *params, double *ms_out);
/* Device-to-device stream copy of `bytes` on the handle's stream, `reps` times: measured copy
 * bandwidth in GB/s (read+write bytes / time) -- the "measured HBM peak" of SURVEY.md §8(d). */
int tetsim_measure_copy_bandwidth(int32_t device, uint64_t bytes, uint32_t reps, double *gbps_out);
/* The same probe by kind: 0 = copy (read + write bytes / time, what tetsim_measure_copy_bandwidth returns), 1 = read only, 2 = write
 * only (bytes / time).  Every lane keeps four independent 16-byte accesses in flight; at its first use per (device, kind, size class)
 * the probe times plain and non-temporal accesses at five grid sizes and keeps the fastest -- a yardstick has to be the best the
 * chip does, not one guess at it (MI355X_MICROARCH.md "HBM": ~6.3 TB/s achievable for a float4 copy). */
int tetsim_measure_stream_bandwidth(int32_t device, uint64_t bytes, uint32_t reps, int32_t kind, double *gbps_out);

/* --- multi-GPU halo (POLAR_JACOBI, part_count > 1) ---------------------------------------------- */

/* RCCL transport: rank 0 calls tetsim_comm_unique_id, the host distributes the 128 bytes, every rank
 * calls tetsim_comm_init.  Afterwards tetsim_step/_step_n exchange ghost positions with neighbouring
 * partitions every substep (grouped ncclSend/ncclRecv on a dedicated stream).
 * Deployment assumption: ONE PROCESS PER GPU stepping ONE partitioned body.  tetsim_step_n replays the two queues' kernel
 * chains from captured graphs that wait for each other through device words, which is only live while the handle's two
 * streams are served by independent hardware queues.  That is probed per body, again whenever this library has created
 * another stream in the process, and a timed-out wait disables replay for good (tetsim_sync) -- but streams that other code
 * creates in the same process are invisible to the probe.  TETSIM_HALO_GRAPH=0 keeps the halo path eager, which is live on
 * any queue mapping. */
int tetsim_comm_unique_id(void *id128);
int tetsim_comm_init(tetsim_handle h, const void *id128, int32_t rank, int32_t nranks);
/* What RCCL itself says about this handle's communicator (ncclCommCount / ncclCommUserRank) -- not what the caller passed to
 * tetsim_comm_init -- plus the halo this partition moves per substep: neighbours, bytes sent to and received from all of them,
 * and the largest single message.  bench.py puts it in its JSON line and refuses to report a run whose ranks != --gpus. */
typedef struct TetSimCommInfo {
    int32_t rccl_ranks, rccl_rank;
    uint32_t neighbours;
    uint64_t send_bytes_per_substep, recv_bytes_per_substep, max_message_bytes;
    int32_t loopback;            /* TETSIM_DEBUG_LOOPBACK_HALO: the halo partner is this rank itself (measurement only) */
    int32_t p2p;                 /* 1: the per-substep halo is stored straight into the neighbours' ghost ranges (tetsim_halo_p2p_connect);
                                    occupies what was tail padding: the struct's size is unchanged */
} TetSimCommInfo;
int tetsim_comm_info(tetsim_handle h, TetSimCommInfo *out);
/* Send 1 KiB to this handle's own rank and receive it back through the initialised communicator, on the halo
 * stream, and verify the bytes: exercises the run-time-resolved RCCL entry points on hosts with a single GPU. */
int tetsim_comm_selftest(tetsim_handle h);
/* Measurement helper: `reps` grouped ncclSend+ncclRecv of `bytes` to this rank itself on the halo stream, issued eagerly
 * (use_graph = 0) or captured per_graph at a time into a HIP graph and replayed (use_graph = 1); checks the bytes.
 * host_us = host time to issue one group, total_us = wall time per group.  Design input for DESIGN.md 7. */
int tetsim_comm_probe(tetsim_handle h, uint64_t bytes, uint32_t reps, int32_t use_graph, uint32_t per_graph,
                      double *host_us, double *total_us);
/* What one halo exchange costs this rank with ITS neighbours and message sizes: `reps` grouped send / recv of the current predictions
 * into the neighbours' ghost ranges (idempotent), each bracketed by events on the halo stream; min / median / max in microseconds.
 * A collective of all ranks (same reps), between steps.  The transfer term of the substep's halo chain, measured on the real wire
 * (bench.py --gpus N reports it per rank).  Since ABI 4. */
int tetsim_halo_probe(tetsim_handle h, uint32_t reps, double *min_us, double *median_us, double *max_us);
/* Peer-to-peer halo (opt-in; POLAR_JACOBI + TETSIM_FAST blocked partitions).  The per-substep ghost exchange without a transfer
 * kernel: each rank's boundary-particle kernel stores its new predictions straight into the neighbours' ghost ranges (peer memory
 * over xGMI, mapped through HIP IPC; double buffered by substep parity) and a word per neighbour says "arrived"; the halo-side
 * tiles wait for those words.  RCCL's grouped send/recv kernel (~15 us even to itself) leaves the substep's critical chain.
 *   every rank:  tetsim_halo_p2p_export(h, blob)            -> TETSIM_P2P_BLOB_BYTES bytes describing its buffers
 *   the host:    gathers the blobs of all part_count ranks (any transport: torch.distributed, MPI, files)
 *   every rank:  tetsim_halo_p2p_connect(h, blobs, part_count)   [blobs + r * TETSIM_P2P_BLOB_BYTES = rank r's]
 * Ranks of the same process connect through plain pointers and must be stepped TOGETHER with tetsim_group_step_n (after its first
 * call): their kernels wait for each other on the device, which is only live if no wait is submitted in front of the kernel that
 * satisfies it -- the group call orders the submissions, independent tetsim_step_n calls of two bodies of one process do not.  A
 * loopback body (TETSIM_DEBUG_LOOPBACK_HALO) connects to itself with its own blob (count 1).  Call between steps, and before ANY rank
 * steps again (the host synchronises the ranks around it).  On top of an RCCL communicator (connect after tetsim_comm_init) RCCL keeps
 * carrying the one refresh exchange after a dt change; without one the peer-to-peer halo is the only transport and dt must stay fixed.
 * Device-side waits are bounded by TETSIM_HALO_TIMEOUT_MS as read at this call.  Results are the RCCL transport's, bit for bit. */
#define TETSIM_P2P_BLOB_BYTES 512
int tetsim_halo_p2p_export(tetsim_handle h, void *blob);
int tetsim_halo_p2p_connect(tetsim_handle h, const void *blobs, uint32_t count);
/* tetsim_halo_probe's counterpart for the peer-to-peer halo (since ABI 5): `reps` hand-overs with all neighbours at once -- one store
 * into each neighbour's inbox word, one wait on the own ones, on the halo stream -- timed by the device's wall clock; min / median / max
 * microseconds per hand-over (one one-way signal latency of this wire; the boundary predictions ride with the same kind of stores).
 * A collective of all ranks (same reps, the same number of calls), between steps; one-layer ghost regions only. */
int tetsim_halo_p2p_probe(tetsim_handle h, uint32_t reps, double *min_us, double *median_us, double *max_us);
/* All partitions of one decomposition living in ONE process (one or several devices): n substeps with the SAME
 * stream/event choreography as the RCCL path -- interior tiles, wait for the previous halo, boundary tiles, boundary
 * particles, start the halo on a second stream, interior particles -- with asynchronous device copies standing in
 * for ncclSend/ncclRecv.  handles[i] must be partition i.  Asynchronous; reads synchronise.  The first call wires the members to
 * each other (plain pointers); tetsim_destroy of a member first drains its siblings' queues (their transfers land in its ghost ranges)
 * and the siblings forget it: they can still be read, saved and destroyed, a later tetsim_group_step_n with them is TETSIM_ESTATE
 * (create the partitions anew).  On failure tetsim_last_error(NULL) has the failing member's text. */
int tetsim_group_step_n(tetsim_handle *handles, uint32_t count, uint32_t n, double dt, const TetSimParams *params);
/* In-process transport for partitions living on one device (tests; "multi-GPU without a cluster"):
 * after every handle has been stepped ONE substep, copy owned interface positions into the
 * neighbours' ghost ranges.  handles[i] must be partition i of the same mesh. */
int tetsim_halo_exchange_local(tetsim_handle *handles, uint32_t count);
/* Host-visible halo plan of this handle (for transports implemented by the caller and for tests):
 * neighbour ranks, and per neighbour the global ids sent and received, concatenated. */
int tetsim_get_halo_plan(tetsim_handle h, int32_t *neigh /*[num_neighbours]*/,
                         int32_t *send_counts, int32_t *recv_counts,
                         int32_t *send_ids, int32_t *recv_ids);
/* Export this handle's packed send buffer for neighbour slot `n` (device->host) / import a received
 * one (host->device): the slow, transport-agnostic path used by the CPU `gloo` tests. */
int tetsim_halo_export(tetsim_handle h, uint32_t n, float *out_xyzw);
int tetsim_halo_import(tetsim_handle h, uint32_t n, const float *in_xyzw);

/* --- host-side preprocessing, callable without a GPU (unit-tested on CPU) ------------------------ */

/* Dependency levels of sequential Gauss-Seidel over `tets` in the given order: level[e] in [0,L).
 * Tets of one level are vertex-disjoint and every pair sharing a vertex keeps its relative order. */
int tetsim_prep_levels(const int32_t *tets, uint32_t nt, uint32_t nv, int32_t *level, uint32_t *num_levels);
/* Greedy colouring in tet order (smallest colour not used by any tet sharing a vertex). */
int tetsim_prep_colours(const int32_t *tets, uint32_t nt, uint32_t nv, int32_t *colour, uint32_t *num_colours);
/* The TETSIM_ORDER_CLUSTERED schedule of a mesh.  order[i] = caller's tet id at sequential position i (what
 * tetsim_get_tet_order returns for such a body); launch[i] / lane[i] / step[i] = the kernel launch (cluster colour), the lane
 * (cluster) and the lane's step that solve position i.  Correct iff any two positions a < b whose tets share a vertex have
 * launch[a] < launch[b], or the same launch AND lane with step[a] < step[b]. */
int tetsim_prep_clusters(const int32_t *tets, uint32_t nt, uint32_t nv, int32_t *order, int32_t *launch, int32_t *lane,
                         int32_t *step, uint32_t *num_launches, uint32_t *num_clusters);
/* The tile plan of the blocked polar kernels for a mesh or a batch of meshes (body_first_tet / body_first_vert
 * [bodies + 1] as tetsim_create_batch lays them out; NULL = one body): tets in tile order (tile_tets[i] = input tet at position
 * i), tile offsets into it (tile_off [tiles + 1]; pass NULL arrays to query *num_tiles first: at most nt of them), and per
 * position the tile-local particle slot of each corner (corner_slot [4 * nt], < 256).  Host only; what the property tests check:
 * <= 256 tets and <= 256 particles per tile, every tet in exactly one tile, no tile spanning two bodies, a body tiled in a batch
 * exactly as alone. */
int tetsim_prep_tiles(const float *verts, uint32_t nv, const int32_t *tets, uint32_t nt, const uint32_t *body_first_tet,
                      const uint32_t *body_first_vert, uint32_t bodies, int32_t *tile_tets, uint32_t *tile_off,
                      uint8_t *corner_slot, uint32_t *num_tiles);
/* The tables behind a tile's fixed reduction order, for a mesh tiled as tetsim_prep_tiles tiles one body (ref_table != 0: with the
 * reference's 36-slot scatter table deciding which (tet, corner) pairs count, quirk and cap included; 0: all of them).  sizes =
 * {tiles, tile slots}; pass NULL arrays to query them first.  tile_tets [nt], tile_off [tiles + 1] and corner_slot [4 * nt] as
 * tetsim_prep_tiles gives them; slot_off [tiles + 1] and slot_particle [slots]: the particles of each tile's slots.  The order in two
 * forms.  (1) entries [4 * nt] and ranges [slots], what the four-lane kernels of small bodies read: tile b's entries start at
 * 4 * tile_off[b]; slot g adds entries [ranges[g] & 0x7ff, ranges[g] >> 16) of its tile, an entry being corner * 256 + tet (the tet's
 * position in the tile); bit 15 of ranges[g]: the slot is the first on its particle's list (it writes the particle back).  Only pairs
 * that count have an entry.  (2) tet_pos [2 * nt] and run_first [slots + tiles], what the 256-tet kernels read: a tile's LIST holds
 * every pair of the tile, sorted by slot -- a slot's counted pairs first and in the order of (1), the others behind them; tet
 * position i has corner k at list position (tet_pos[2 i] | (uint64_t)tet_pos[2 i + 1] << 32) >> 10 k & 1023, bit 40 + k set if that
 * pair does not count (the kernels add +0 for it); slot g of tile b has the run [run_first[g + b] & 0x7ff, run_first[g + b + 1] &
 * 0x7ff), the tile's last entry being the list's length, and bit 15 as in (1). */
int tetsim_prep_tile_tables(const float *verts, uint32_t nv, const int32_t *tets, uint32_t nt, int32_t ref_table, uint32_t sizes[2],
                            int32_t *tile_tets, uint32_t *tile_off, uint32_t *slot_off, int32_t *slot_particle, uint8_t *corner_slot,
                            uint16_t *entries, uint32_t *ranges, uint32_t *tet_pos, uint16_t *run_first);
/* The routine behind tetsim_set_colliders and tetsim_set_body_colliders, without a device, for tests (as_rows != 0: every field rounded to
 * f32 first and taken from there, as a row of tetsim_set_body_colliders holds it): per collider codes[k] = 0, or why
 * it is refused -- 1 unknown kind, 2 non-finite value, 3 negative radius or friction, 4 zero-length plane normal, 5 negative half-extent,
 * 6 zero-length box axis, 7 box axes not orthogonal, the first that applies (`reserved` is not looked at) -- and the bytes of the two views
 * the kernels read, zeros for a refused collider: views_f64 [count] records of a[3], b[3], u[9], radius, friction, v[3] as double, then
 * kind and 0 as int32; views_f32 [count] the same with float. */
#define TETSIM_COLLIDER_VIEW_F64_BYTES 168
#define TETSIM_COLLIDER_VIEW_F32_BYTES 88
int tetsim_prep_collider_views(const TetSimCollider *colliders, uint32_t count, int32_t as_rows, int32_t *codes, void *views_f64, void *views_f32);
/* Scatter table of SoftbodyGPU.js:563-577: slots[v*36 + s] = 4*tet + corner, -1 = empty.
 * ref_quirk != 0 reproduces the `<= 0.0` test.  Returns the number of dropped contributions. */
/* The topology of that tree for any triangle list, without a device: positions [3 * nvis], tri_ids [3 * ntri], tri_body [ntri] (the
 * body of every triangle) or NULL for one body.  tri_first [bodies + 1]: the bodies' ranges in `order`; order [ntri]: triangle ids, per
 * body in Morton order; leaf l of body b holds order[tri_first[b] + 4 l ...] (four, fewer at the end); node_first [bodies + 1] and depth
 * [bodies]: body b has 2^depth leaf slots and its node i (root 1, children 2 i and 2 i + 1, leaves from 2^depth) is slot
 * node_first[b] + i.  node_range, if not NULL: [node_first[bodies]][2], per slot the range in `order` of the triangles below it. */
int tetsim_prep_bvh(const float *positions, uint32_t nvis, const int32_t *tri_ids, uint32_t ntri, const int32_t *tri_body, uint32_t bodies,
                    uint32_t *tri_first, uint32_t *order, uint32_t *node_first, uint32_t *depth, uint32_t *node_range);
int tetsim_prep_slot_table(const int32_t *tets, uint32_t nt, uint32_t nv, int32_t ref_quirk,
                           int32_t *slots /*[nv*36]*/, uint32_t *dropped);
/* The dispatch schedule of the one-launch polar call (large unpartitioned bodies, fused_particle_pass 5).  Host only.
 * tetsim_prep_call_tiles: what the schedule is built from, for a mesh tiled as tetsim_create tiles an unpartitioned body (particles in
 * the device's numbering): sizes = {tiles, tile slots, vp_cols, nv_pad}; blk_vert_off [tiles + 1] and blk_verts [slots]: the particles
 * each tile stages; vp_ell [vp_cols * nv_pad]: per particle v the tile slots on its lists, vp_ell[j * nv_pad + v], 0xffffffff = none.
 * Pass NULL arrays to query the sizes first.
 * tetsim_prep_call_schedule: one periodic table of *period entries (a multiple of 8); block g of a call of n substeps runs entry
 * g % period for substep g / period (one less for a WRAPPED entry; a substep outside [0, n) does nothing), n * period + *tail blocks in
 * all.  An entry is kind << 30 | wrapped << 29 | index: kind 0 = a tile, index = its block r in the plain order (tile
 * (r % 8) * ceil(tiles / 8) + r / 8, always at a position = r mod 8); 1 = particles [256 * index, 256 * index + 256); 2 = nothing.
 * lag 0 = the plain order, every tile and then every particle block; lag L = a particle block 8 * L positions behind the last tile on
 * its particles' lists.  A lag that cannot be laid out gives the plain order: *fell_back = 1, the reason in tetsim_last_error(NULL).
 * entry == NULL queries *period (capacity: the entries `entry` has room for).
 * tetsim_prep_check_call_schedule: 0 if whatever a block of the table waits for has a smaller grid index and every tile and particle
 * block appears exactly once, tiles on their XCD in order; else TETSIM_EINVAL and what is wrong in tetsim_last_error(NULL). */
int tetsim_prep_call_tiles(const float *verts, uint32_t nv, const int32_t *tets, uint32_t nt, uint32_t sizes[4],
                           uint32_t *blk_vert_off, int32_t *blk_verts, uint32_t *vp_ell);
int tetsim_prep_call_schedule(const int32_t *blk_verts, const uint32_t *blk_vert_off, uint32_t nb, const uint32_t *vp_ell,
                              uint32_t vp_cols, uint32_t nv_pad, uint32_t nv_owned, uint32_t lag, uint32_t *entry,
                              uint32_t capacity, uint32_t *period, uint32_t *tail, int32_t *fell_back);
int tetsim_prep_check_call_schedule(const int32_t *blk_verts, const uint32_t *blk_vert_off, uint32_t nb, const uint32_t *vp_ell,
                                    uint32_t vp_cols, uint32_t nv_pad, uint32_t nv_owned, const uint32_t *entry, uint32_t period,
                                    uint32_t tail);
/* The particle(s) SoftbodyGPU.js:335-338,345 pins for `grab_id` on a mesh with num_elems tets (texture side
 * ceil(sqrt(num_elems))): out[0..1], -1 = none.  What TETSIM_FLAG_REF_GRAB_TEXEL uses. */
int tetsim_prep_ref_grab_texels(int32_t grab_id, uint32_t num_elems, uint32_t num_particles, int32_t out[2]);
/* A visual mesh for a body WITHOUT an artist's mesh (Softbody.js:46-50 take one from the caller): the tet mesh's boundary faces
 * -- faces of exactly one tet -- oriented outward (counter-clockwise seen from outside: the normal points away from the tet's
 * opposite corner in the rest configuration `verts`; verts == NULL, or a zero-volume tet: the tet is taken as positively
 * oriented, det[v1-v0, v2-v0, v3-v0] > 0, the convention of initPhysics, Softbody.js:69-72), in the reference's own format: one row
 * (tetNr, b0, b1, b2) per boundary VERTEX with one barycentric weight equal to 1 (its skinned position is the particle's position),
 * and triangles over those rows.  Rows ascend by particle id (tetNr = the lowest tet containing it), triangles by (tet, face;
 * face k lies opposite corner k).  *nrows / *ntri receive the counts; vis_verts / tri_ids may both be NULL to query them.  Host only. */
int tetsim_prep_boundary_surface(const float *verts /* [3*nv] rest positions, or NULL */,
                                 const int32_t *tets, uint32_t nt, uint32_t nv,
                                 float *vis_verts /*[4*nrows]*/, int32_t *tri_ids /*[3*ntri]*/,
                                 uint32_t *nrows, uint32_t *ntri);
/* Rest data of Softbody.js:60-87 in JS number semantics: invMass[nv], invRestPose[9*nt] (column-major),
 * invRestVolume[nt]. */
int tetsim_prep_rest(const float *verts, uint32_t nv, const int32_t *tets, uint32_t nt, double density,
                     float *inv_mass, float *inv_rest_pose, float *inv_rest_volume);

/* The built-in vertex partitioner for general meshes (SURVEY.md 8(e) "General meshes: host-side graph partition"; the coupling a cut
 * must respect is the particle -> incident tets table of SoftbodyGPU.js:563-577 that the Jacobi average :306-319 reads): which
 * partition owns each particle, vert_owner_out [nv], values in [0, part_count).  Recursive bisection at the weighted median
 * (weights 1 + valence: a part's tets ~ the corners it owns / 4) of the key that cuts the fewest tets -- breadth-first distances
 * from the two ends of a pseudo-diameter and their difference (topology only), plus x / y / z when `verts` is not NULL -- then
 * k-way boundary refinement (a particle moves to the part holding more of its tet-mates) which keeps every part within +-3% of the
 * mean weight of what the cuts gave it (a cut lands on a particle boundary: one particle's weight per bisection level on top, which
 * only shows on meshes of a few dozen particles).  Deterministic.  tetsim_create and tetsim_plan_create* with part_count > 1 and vert_owner == NULL use this WITHOUT
 * coordinates (verts == NULL: the plan entry points have none, and a plan must equal what tetsim_create builds); pass the
 * result of a call WITH coordinates as vert_owner to both for planar cuts on lattice-like meshes, or store it in a .tetsim
 * container (TetSimMeshArrays.vert_owner). */
int tetsim_prep_partition(const float *verts /* [3*nv] or NULL */, uint32_t nv, const int32_t *tets, uint32_t nt,
                          int32_t part_count, int32_t *vert_owner_out);
/* What a particle -> partition map costs, per partition (out [part_count]; the counts the partition plans would have, without
 * building them).  vert_owner == NULL: the map tetsim_create would pick itself.  Ghost-particle fraction of partition r =
 * ghost_particles / (owned_particles + ghost_particles) -- what crosses the wire per substep against what is integrated --,
 * ghost-tet fraction = (local_elems - owned_elems summed over r) / num_elems -- the tets solved twice. */
typedef struct TetSimPartQuality {
    uint32_t owned_particles;    /* particles this partition integrates */
    uint32_t ghost_particles;    /* particles it reads but does not own (received every substep) */
    uint32_t boundary_particles; /* owned particles some other partition reads (sent every substep) */
    uint32_t local_elems;        /* tets it solves: every tet touching an owned particle */
    uint32_t owned_elems;        /* tets counted once across partitions (lowest-owner rule) */
    uint32_t num_neighbours;
} TetSimPartQuality;
int tetsim_prep_partition_quality(const int32_t *tets, uint32_t nt, uint32_t nv, int32_t part_count,
                                  const int32_t *vert_owner, TetSimPartQuality *out);

/* Domain-decomposition plan of one partition, computed on the host exactly as tetsim_create does for
 * part_count > 1 (local numbering: owned boundary | owned interior | ghosts grouped by owner).  Lets a host
 * drive its own transport and lets the multi-process path be tested without GPUs. */
typedef struct tetsim_plan_s *tetsim_plan;
typedef struct TetSimPlanSizes {
    uint32_t owned_particles, boundary_particles, local_particles, local_elems, owned_elems, num_neighbours;
} TetSimPlanSizes;
int tetsim_plan_create(const int32_t *tets, uint32_t nt, uint32_t nv, int32_t part_count, int32_t part_index,
                       const int32_t *vert_owner, tetsim_plan *out);
/* The same plan with a ghost region `depth` layers deep (1 or 2).  Depth 2: the second layer holds the particles that share a tet
 * with a first-layer ghost, the local tets include the tets of the first-layer ghosts that touch no owned particle, and every
 * neighbour has a second pair of lists -- what lets a partition advance its first ghost layer itself and exchange ghosts only every
 * other substep (exercised on the CPU by tests/test_partition_gloo.py).  Local numbering: owned boundary | owned
 * interior | first-layer ghosts by owner | second-layer ghosts by owner. */
int tetsim_plan_create_deep(const int32_t *tets, uint32_t nt, uint32_t nv, int32_t part_count, int32_t part_index,
                            const int32_t *vert_owner, int32_t depth, tetsim_plan *out);
/* first_layer_ghosts: ghosts [owned, owned + that) are the first layer; tet_layer [local_elems]: 0 = touches an owned particle, 1 = not */
int tetsim_plan_layers(tetsim_plan p, uint32_t *first_layer_ghosts, uint8_t *tet_layer);
/* neighbour i's SECOND-layer lists (disjoint from the first-layer ones of tetsim_plan_neighbour) */
int tetsim_plan_neighbour_layer2(tetsim_plan p, uint32_t i, uint32_t *send_count, uint32_t *recv_start, uint32_t *recv_count);
int tetsim_plan_neighbour_layer2_ids(tetsim_plan p, uint32_t i, int32_t *send_local, int32_t *send_global, int32_t *recv_global);
void tetsim_plan_destroy(tetsim_plan p);
int tetsim_plan_sizes(tetsim_plan p, TetSimPlanSizes *out);
/* local_to_global_vert [local_particles], local_to_global_tet [local_elems], local_tets [4*local_elems] */
int tetsim_plan_arrays(tetsim_plan p, int32_t *local_to_global_vert, int32_t *local_to_global_tet, int32_t *local_tets);
/* neighbour i: its rank, how many owned particles are sent to it, and the contiguous local ghost range
 * [recv_start, recv_start+recv_count) its particles are received into. */
int tetsim_plan_neighbour(tetsim_plan p, uint32_t i, int32_t *rank, uint32_t *send_count, uint32_t *recv_start,
                          uint32_t *recv_count, int32_t *send_is_contiguous);
/* send_local / send_global [send_count] (ascending global id), recv_global [recv_count] */
int tetsim_plan_neighbour_ids(tetsim_plan p, uint32_t i, int32_t *send_local, int32_t *send_global, int32_t *recv_global);

int tetsim_abi_version(void);
/* What exactly is loaded.  source_sha: first 16 hex digits of the SHA-256 over the library's sources (csrc/, include/) and
 * build flags, stamped by tetsim_amd/build.py; kernel_sha: the same over the files that determine the polar tet kernel and
 * its tiling (what profiles/pmc_traffic.json is keyed by); ablation != 0: the development build (-DTETSIM_ABLATION) whose
 * tet kernel obeys TETSIM_DEBUG_ITERS / _SKIP_REST_STORE / _NO_PEEL -- never the product; debug_env: bit i set = the i-th of
 * {TETSIM_DEBUG_LOOPBACK_HALO, TETSIM_DEBUG_LOOPBACK_COPY, TETSIM_DEBUG_ONE_STREAM, TETSIM_DEBUG_GROUP_SYNC,
 * TETSIM_DEBUG_HOSTPROF, TETSIM_DEBUG_TRACE*, TETSIM_HALO_SYNC, TETSIM_HALO_GRAPH, TETSIM_DEBUG_LOOPBACK_DELAY_US, TETSIM_NH_QUADS*,
 * TETSIM_FUSED_PARTICLE_PASS, TETSIM_FRAME_KERNEL, TETSIM_FRAME_LOCAL*, TETSIM_NH_FOLD*, TETSIM_HALO_ALIGNED_TILES*, TETSIM_HALO_FOLD_WAIT, TETSIM_QUAD,
 * TETSIM_QUAD_POLL_DELAY*, TETSIM_NH_FRAME*, TETSIM_NH_ONE_LAUNCH, TETSIM_PJ_ONE_LAUNCH, TETSIM_PJ_CALL_LAG} is set in the environment and
 * READ by this build -- the names marked * are A/B switches
 * of choices settled by measurement, which only the development build looks at (the product library reads the 15 others and
 * TETSIM_RCCL_LIB, TETSIM_HALO_TIMEOUT_MS, TETSIM_DEBUG_STREAM_PROBE: INTEGRATION.md 4).  bench.py records all of it in its JSON line. */
typedef struct TetSimLibraryInfo {
    int32_t abi;
    int32_t ablation;
    uint32_t debug_env;
    char source_sha[20];
    char kernel_sha[20];
} TetSimLibraryInfo;
int tetsim_library_info(TetSimLibraryInfo *out);

/* --- .tetsim mesh container (GPU-free except tetsim_create_from_file) ---------------------------
 * The five arrays of the reference's Dragon.js (:1 verts, :311 tetIds, :1080 tetEdgeIds, :1705 attachedVerts
 * [tetNr,b0,b1,b2], :11640 attachedTriIds) as raw little-endian sections of one mmap-able file, plus optional
 * preprocessing: a tet colouring and a vertex->partition map.  Layout in tetsim_amd/csrc/mesh_file.cpp. */
typedef struct TetSimMeshArrays {
    uint32_t num_particles;      /* verts        [3 * num_particles] f32  (required) */
    uint32_t num_elems;          /* tets         [4 * num_elems]     i32  (required, may be empty) */
    uint32_t num_edges;          /* edge_ids     [2 * num_edges]     i32  or NULL */
    uint32_t num_vis_verts;      /* vis_verts    [4 * num_vis_verts] f32  or NULL */
    uint32_t num_vis_tris;       /* vis_tri_ids  [3 * num_vis_tris]  i32  or NULL */
    uint32_t part_count;         /* partitions addressed by vert_owner (0 when absent) */
    const float *verts;
    const int32_t *tets;
    const int32_t *edge_ids;
    const float *vis_verts;
    const int32_t *vis_tri_ids;
    const int32_t *tet_colour;   /* [num_elems] or NULL */
    const int32_t *vert_owner;   /* [num_particles], values in [0, part_count), or NULL */
} TetSimMeshArrays;
typedef struct tetsim_mesh_file *tetsim_mesh;

/* Write `a` to `path` (atomically: temp file + rename). */
int tetsim_mesh_write(const char *path, const TetSimMeshArrays *a);
/* Map a file read-only and validate it (magic, version, bounds, index ranges).  The arrays returned by
 * tetsim_mesh_arrays point INTO the mapping and stay valid until tetsim_mesh_close. */
int tetsim_mesh_open(const char *path, tetsim_mesh *out);
int tetsim_mesh_arrays(tetsim_mesh m, TetSimMeshArrays *out);
int tetsim_mesh_close(tetsim_mesh m);
/* tetsim_create from a file: vertices/tets from the mapping; a stored colouring is used when opts->tet_colour is NULL
 * and the solver/order take one; a stored partition map is used when opts->part_count > 1, opts->vert_owner is NULL
 * and the stored part_count matches; a stored visual mesh is attached (tetsim_set_visual_mesh; partitions keep their rows). */
int tetsim_create_from_file(const char *path, const TetSimOptions *opts, tetsim_handle *out);

#ifdef __cplusplus
}
#endif
#endif /* TETSIM_H */
