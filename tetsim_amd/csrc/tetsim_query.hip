// tetsim_query.hip -- C ABI, part 3b (include/tetsim.h): queries on the skinned visual mesh.  Picking (three.js r160 ray casts from host
// arrays, the bounding sphere), the range sensors (the same casts per body from and into the caller's device memory: brute force or through
// the refitted tree), closest points through that tree (device and host variants), the tree's host side (its tables, tetsim_prep_bvh, the
// development entries of TETSIM_BVH_STATS builds) and the per-body spheres.  Kernels: query_kernels.hip, query_bvh.hip, query_closest.hip.
#include "body_rows.h"

using namespace tetsim;

namespace {
static_assert(sizeof(TetSimRay) == sizeof(RayIn) && sizeof(TetSimRayHit) == sizeof(RayOut), "the ABI's ray records are the kernels' records");
static_assert(sizeof(TetSimPointQuery) == sizeof(PointQueryIn) && sizeof(TetSimClosest) == sizeof(ClosestOut), "the ABI's query records are the kernel's records");
const char* const kPartitionedQuery = "a partition skins only its own rows, and a triangle's corners may belong to other ranks: ray casts and the bounding sphere "
                                      "of a partitioned body are not supported (put the ranks' skins together with tetsim_read_visual_mesh + tetsim_get_visual_ids)";

int check_query_state(tetsim_body* h, bool need_triangles) {
    if (!h->vis_attached) return fail(h, TETSIM_ESTATE, "no visual mesh attached (tetsim_set_visual_mesh)");
    if (need_triangles && (!h->skin.vt_off || h->skin.ntri == 0)) return fail(h, TETSIM_ESTATE, "no visual triangles attached (tetsim_set_visual_triangles)");
    if (h->partitioned) return fail(h, TETSIM_ESTATE, kPartitionedQuery);
    if (h->skin.nvis == 0) return fail(h, TETSIM_ESTATE, "the visual mesh has no vertices");
    return 0;
}

// ---- the tables of a handle's visual mesh (query_device.h), built and uploaded once -------------------------------------------------------
// of the visual rows: the body of every row, the rows of every body, the sphere keys
int ensure_row_tables(tetsim_body* h) {
    if (h->qrows_ready) return 0;
    QueryBodiesDev& b = h->qbodies;
    const uint32_t nb = h->info.num_bodies, nvis = h->skin.nvis;
    std::vector<uint32_t> row_body(nvis, 0u), body_rows(nb, 0u);
    for (uint32_t i = 0; i < nvis; i++) {
        if (!h->vis_row_body.empty()) row_body[i] = static_cast<uint32_t>(h->vis_row_body[i]);
        body_rows[row_body[i]]++;
    }
    uint32_t *d_row_body = nullptr, *d_body_rows = nullptr;
    if (int rc = dev_alloc(h, &d_row_body, row_body.size())) return rc;
    if (int rc = dev_alloc(h, &d_body_rows, body_rows.size())) return rc;
    if (int rc = dev_alloc(h, &b.spheres, static_cast<size_t>(nb) * kSphereWords)) return rc;
    if (int rc = upload(h, d_row_body, row_body)) return rc;
    if (int rc = upload(h, d_body_rows, body_rows)) return rc;
    b.bodies = nb; b.row_body = d_row_body; b.body_rows = d_body_rows;
    h->qrows_ready = true;
    return 0;
}

// The triangle ids stably sorted by body (a body's triangles in list order) with the bodies' offsets; tri_body null: one body.  *most, if
// not null: the triangles of the largest body.
void sort_triangles_by_body(const int32_t* tri_body, uint32_t ntri, uint32_t bodies, std::vector<uint32_t>* first, std::vector<uint32_t>* sorted, uint32_t* most) {
    auto body_of = [&](uint32_t t) { return tri_body ? static_cast<uint32_t>(tri_body[t]) : 0u; };
    first->assign(bodies + 1u, 0u);
    sorted->resize(ntri);
    for (uint32_t t = 0; t < ntri; t++) (*first)[body_of(t) + 1u]++;
    uint32_t largest = 0;
    for (uint32_t k = 0; k < bodies; k++) { largest = std::max(largest, (*first)[k + 1u]); (*first)[k + 1u] += (*first)[k]; }
    std::vector<uint32_t> fill(first->begin(), first->end() - 1);
    for (uint32_t t = 0; t < ntri; t++) (*sorted)[fill[body_of(t)]++] = t;   // (in list order: stable)
    if (most) *most = largest;
}

// ... and of the triangle list: the sort above, the body of every triangle (batches), the candidates of the few-ray launches.  (A triangle
// whose rows belong to different bodies was found by tetsim_set_visual_triangles: tri_spans_bodies.)
int ensure_triangle_tables(tetsim_body* h) {
    if (h->qtris_ready) return 0;
    if (int rc = ensure_row_tables(h)) return rc;
    QueryBodiesDev& b = h->qbodies;
    std::vector<uint32_t> first, sorted;
    uint32_t most = 0;
    sort_triangles_by_body(h->tri_body.empty() ? nullptr : h->tri_body.data(), h->skin.ntri, b.bodies, &first, &sorted, &most);
    uint32_t *d_sorted = nullptr, *d_first = nullptr;
    int32_t* d_tri_body = nullptr;
    if (int rc = dev_alloc(h, &d_sorted, sorted.size())) return rc;
    if (int rc = dev_alloc(h, &d_first, first.size())) return rc;
    if (int rc = dev_alloc(h, &h->d_cast_cand, kCastCandCap)) return rc;
    if (int rc = upload(h, d_sorted, sorted)) return rc;
    if (int rc = upload(h, d_first, first)) return rc;
    if (!h->tri_body.empty()) {
        if (int rc = dev_alloc(h, &d_tri_body, h->tri_body.size())) return rc;
        if (int rc = upload(h, d_tri_body, h->tri_body)) return rc;
    }
    b.tri_sorted = d_sorted; b.tri_first = d_first; b.tri_body = d_tri_body;
    b.max_tiles = std::max((most + kCastTile - 1u) / kCastTile, 1u);
    h->qtris_ready = true;
    return 0;
}

// ---- skinning and spheres in front of every query ------------------------------------------------------------------------------------------
// what the query kernels read of a handle: the skinned rows, the triangles, the sphere keys
QueryDev query_view(const tetsim_body* h) {
    QueryDev q;
    q.nvis = h->skin.nvis; q.ntri = h->skin.ntri; q.pos = h->skin.out_pos; q.tri = h->skin.tri; q.sphere = h->d_sphere;
    return q;
}

// skinning alone: the visual positions of the last enqueued substep in skin.out_pos, on h->stream
int skin_for_query(tetsim_body* h, QueryDev* q) {
    const bool pjs = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI;
    if (pjs) { if (int rc = ensure_quats(h)) return rc; }
    if (!h->d_sphere) { if (int rc = dev_alloc(h, &h->d_sphere, kSphereWords)) return rc; }
    skin_launch(h->stream, h->skin, pjs ? h->pj.pos_final : h->nh.pos, pjs ? h->pj.quat : nullptr, !pjs);
    *q = query_view(h);
    return 0;
}

enum class Spheres { kMesh, kBodies };   // the keys a call reads: the whole mesh's, or every body's (records that name their bodies)
void launch_spheres(tetsim_body* h, const QueryDev& q, Spheres spheres) {
    if (spheres == Spheres::kBodies) query_launch_body_spheres(h->stream, q, h->qbodies);
    else query_launch_sphere(h->stream, q);
}

// the visual positions of the last completed substep in skin.out_pos and their bounding sphere in d_sphere, on h->stream
int skin_and_sphere(tetsim_body* h, QueryDev* q) {
    HIPCHK(h, hipSetDevice(h->opt.device));
    if (int rc = skin_for_query(h, q)) return rc;
    launch_spheres(h, *q, Spheres::kMesh);
    return 0;
}

// ---- picking: three.js r160 ray casts of host arrays (query_kernels.hip) ----------------------------------------------------------------------
int check_rays(tetsim_body* h, const TetSimRay* rays, uint32_t count) {
    for (uint32_t i = 0; i < count; i++) {
        // (ray_defect, query_device.h: the one definition of an invalid ray; the device's cast reads it too)
        static const char* const why[] = {"", "non-finite origin or direction", "zero direction", "near or far is NaN", "near < 0", "far < near"};
        const TetSimRay& r = rays[i];
        if (const int defect = ray_defect(r.origin, r.direction, r.near, r.far)) return fail(h, TETSIM_EINVAL, "ray " + std::to_string(i) + ": " + why[defect]);
    }
    return 0;
}

int cast_rays(tetsim_body* h, const TetSimRay* rays, uint32_t count, TetSimRayHit* hits) {
    if (int rc = check_rays(h, rays, count)) return rc;
    QueryDev q;
    HIPCHK(h, hipSetDevice(h->opt.device));
    const uint32_t per_ray = query_blocks_per_ray(h->skin.ntri, count);
    int rc;
    const size_t want = std::max<size_t>(count, 64);   // (one capacity per buffer: a failed allocation leaves the others' bookkeeping right)
    if ((rc = dev_grow(h, &h->d_rays, &h->ray_cap, want)) || (rc = dev_grow(h, &h->d_ray_prep, &h->ray_prep_cap, want)) ||
        (rc = dev_grow(h, &h->d_ray_hits, &h->ray_hits_cap, want))) return rc;
    if ((rc = dev_grow(h, &h->d_ray_cand, &h->ray_cand_cap, static_cast<size_t>(count) * per_ray))) return rc;
    HIPCHK(h, hipMemcpy(h->d_rays, rays, count * sizeof(RayIn), hipMemcpyHostToDevice));
    if ((rc = skin_and_sphere(h, &q))) return rc;
    query_launch_rays(h->stream, q, h->d_rays, h->d_ray_prep, h->d_ray_cand, h->d_ray_hits, count, per_ray);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(hits, h->d_ray_hits, count * sizeof(RayOut), hipMemcpyDeviceToHost));
    if (!h->tri_body.empty())
        for (uint32_t i = 0; i < count; i++)
            if (hits[i].hit) hits[i].body = h->tri_body[hits[i].triangle];
    return 0;
}

// ---- the calls on records: one list of checks, one enqueue -----------------------------------------------------------------------------------
// The topology of the tree (query_device.h), built once from the positions of this moment: the call skins, waits and reads the positions and
// the tables back -- as the first tetsim_raycast_visual_device call blocks for its tables.  Boxes are not made here: every call refits them.
int ensure_bvh(tetsim_body* h) {
    if (h->bvh_ready) return 0;
    if (int rc = ensure_triangle_tables(h)) return rc;
    QueryDev q;
    if (int rc = skin_for_query(h, &q)) return rc;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const QueryBodiesDev& b = h->qbodies;
    std::vector<float4> pos(q.nvis);
    std::vector<int4> tri(q.ntri);
    std::vector<uint32_t> sorted(q.ntri), first(b.bodies + 1u);
    HIPCHK(h, hipMemcpy(pos.data(), q.pos, pos.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(tri.data(), q.tri, tri.size() * sizeof(int4), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(sorted.data(), b.tri_sorted, sorted.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(first.data(), b.tri_first, first.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    BvhTopology topo;
    const std::string why = bvh_build_topology(&pos[0].x, 4u, &tri[0].x, 4u, sorted.data(), first.data(), b.bodies, &topo);
    if (!why.empty()) return fail(h, TETSIM_EINVAL, why);
    uint32_t *d_order = nullptr, *d_node_first = nullptr, *d_depth = nullptr, *d_fold = nullptr, *d_top = nullptr;
    BvhBox* d_box = nullptr;
    int rc;
    if ((rc = dev_alloc(h, &d_order, topo.order.size())) || (rc = dev_alloc(h, &d_node_first, topo.node_first.size())) ||
        (rc = dev_alloc(h, &d_depth, topo.depth.size())) || (rc = dev_alloc(h, &d_fold, topo.fold.size())) ||
        (rc = dev_alloc(h, &d_top, topo.top_body.size())) || (rc = dev_alloc(h, &d_box, topo.node_first[b.bodies]))) return rc;
    if ((rc = upload(h, d_order, topo.order)) || (rc = upload(h, d_node_first, topo.node_first)) || (rc = upload(h, d_depth, topo.depth)) ||
        (rc = upload(h, d_fold, topo.fold)) || (rc = upload(h, d_top, topo.top_body))) return rc;
    BvhDev& v = h->bvh;
    v.order = d_order; v.node_first = d_node_first; v.depth = d_depth; v.box = d_box; v.fold = d_fold; v.top_body = d_top;
    v.folds = static_cast<uint32_t>(topo.fold.size() / 2u); v.tops = static_cast<uint32_t>(topo.top_body.size());
    h->bvh_ready = true;
    return 0;
}

// The records of a call: the nouns of its refusals and the records' sizes.  A call on them: which tables it needs and its kernels.
struct RecordKind {
    const char *in_stride, *out_stride, *in, *out, *body, *without;
    uint64_t in_row, out_row;
};
const RecordKind kRays = {"ray_stride", "hit_stride", "rays", "hits", "ray_body", "cast without ray_body", sizeof(TetSimRay), sizeof(TetSimRayHit)};
const RecordKind kQueries = {"query_stride", "out_stride", "queries", "out", "query_body", "query without query_body", sizeof(TetSimPointQuery), sizeof(TetSimClosest)};
enum class QueryTables { kRows, kTriangles, kTree };   // each holds the one before: the rows' bodies; the sorted triangle list; the tree, refitted by the call
struct RecordCall {
    const RecordKind& kind;
    QueryTables tables;
    void (*launch)(tetsim_body* h, const QueryDev& q, const CastIo& io);
};
const RecordCall kCastBrute = {kRays, QueryTables::kTriangles,
                               [](tetsim_body* h, const QueryDev& q, const CastIo& io) { query_launch_cast_device(h->stream, q, h->qbodies, io, h->d_cast_cand); }};
const RecordCall kCastTree = {kRays, QueryTables::kTree,
                              [](tetsim_body* h, const QueryDev& q, const CastIo& io) { query_launch_cast_bvh(h->stream, q, h->qbodies, h->bvh, io); }};
const RecordCall kClosestTree = {kQueries, QueryTables::kTree,
                                 [](tetsim_body* h, const QueryDev& q, const CastIo& io) { query_launch_closest_bvh(h->stream, q, h->qbodies, h->bvh, io); }};

// what a call on records checks before anything touches the device, in the one order of refusals; *io: the resolved records
int check_records(tetsim_body* h, const RecordKind& c, const void* in, uint64_t in_stride, const void* body, uint32_t count, void* out, uint64_t out_stride, CastIo* io) {
    if (count && (!in || !out)) return fail(h, TETSIM_EINVAL, "null argument");
    if (int rc = check_record_stride(h, c.in_stride, in_stride, c.in_row, 8u)) return rc;
    if (int rc = check_record_stride(h, c.out_stride, out_stride, c.out_row, 8u)) return rc;
    if (int rc = check_query_state(h, true)) return rc;
    if (body && h->tri_spans_bodies)
        return fail(h, TETSIM_ESTATE, std::string("a triangle of the visual mesh has rows of different bodies: it belongs to no body's own surface (") + c.without + ")");
    io->in = static_cast<const char*>(in); io->in_stride = resolved_stride(in_stride, c.in_row);
    io->body = static_cast<const int32_t*>(body);
    io->out = static_cast<char*>(out); io->out_stride = resolved_stride(out_stride, c.out_row);
    io->count = count;
    return 0;
}

// Behind the checks, where only allocation and HIP itself can fail: the tables (only a handle's first tree call blocks), then on the
// handle's stream under the caller's stream contract skinning, the spheres, the refit of a tree call and the caller's launch(q).
template <class Launch>
int enqueue_query(tetsim_body* h, QueryTables tables, Spheres spheres, void* caller_stream, Launch&& launch) {
    const bool tree = tables == QueryTables::kTree;
    if (int rc = tables == QueryTables::kRows ? ensure_row_tables(h) : ensure_triangle_tables(h)) return rc;
    if (tree) { if (int rc = ensure_bvh(h)) return rc; }
    return on_caller_stream(h, caller_stream, [&]() -> int {
        QueryDev q;
        if (int rc = skin_for_query(h, &q)) return rc;
        launch_spheres(h, q, spheres);
        if (tree) query_launch_bvh_refit(h->stream, q, h->qbodies, h->bvh);
        launch(q);
        return launched(h);
    });
}
int enqueue_records(tetsim_body* h, const RecordCall& c, const CastIo& io, void* caller_stream) {
    return enqueue_query(h, c.tables, io.body ? Spheres::kBodies : Spheres::kMesh, caller_stream, [&](const QueryDev& q) { c.launch(h, q, io); });
}

// tetsim_raycast_visual_device, tetsim_raycast_visual_bvh_device and tetsim_closest_visual_device: one signature, one list of errors, one handshake
int records_device_call(tetsim_handle h, const RecordCall& c, const void* in, uint64_t in_stride, const void* body, uint32_t count, void* out, uint64_t out_stride,
                        void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    CastIo io;
    const RecordKind& k = c.kind;
    if (int rc = check_records(h, k, in, in_stride, body, count, out, out_stride, &io)) return rc;
    if (count == 0) return 0;
    if (int rc = device_call_guard(h)) return rc;
    if (int rc = check_device_records(h, in, io.in_stride, count, k.in_row, 8u, k.in)) return rc;
    if (int rc = check_device_records(h, out, io.out_stride, count, k.out_row, 8u, k.out)) return rc;
    if (body) { if (int rc = check_device_records(h, body, 4u, count, 4u, 4u, k.body)) return rc; }
    return enqueue_records(h, c, io, caller_stream);
}
}  // namespace

extern "C" {

int tetsim_raycast_visual(tetsim_handle h, const TetSimRay* rays, uint32_t count, TetSimRayHit* hits) {
    if (!h) return fail(h, TETSIM_EINVAL, "null argument");
    if (count && (!rays || !hits)) return fail(h, TETSIM_EINVAL, "null argument");
    if (int rc = check_query_state(h, true)) return rc;
    if (count == 0) return 0;
    return cast_rays(h, rays, count, hits);
}

int tetsim_read_visual_bounding_sphere(tetsim_handle h, double centre[3], double* radius) {
    if (!h || !centre || !radius) return fail(h, TETSIM_EINVAL, "null argument");
    if (int rc = check_query_state(h, false)) return rc;
    QueryDev q;
    if (int rc = skin_and_sphere(h, &q)) return rc;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    uint32_t words[kSphereWords];
    HIPCHK(h, hipMemcpy(words, h->d_sphere, sizeof(words), hipMemcpyDeviceToHost));
    query_decode_sphere(words, centre, radius);
    return 0;
}

// ---- range sensors: the same casts and spheres per body, from and into the caller's device memory (query_device.h) -------------------
int tetsim_raycast_visual_device(tetsim_handle h, const void* rays, uint64_t ray_stride, const void* ray_body, uint32_t count, void* hits, uint64_t hit_stride,
                                 void* caller_stream) {
    return records_device_call(h, kCastBrute, rays, ray_stride, ray_body, count, hits, hit_stride, caller_stream);
}

// the same casts through the refitted tree (query_bvh.hip); its own definition: include/tetsim.h
int tetsim_raycast_visual_bvh_device(tetsim_handle h, const void* rays, uint64_t ray_stride, const void* ray_body, uint32_t count, void* hits,
                                     uint64_t hit_stride, void* caller_stream) {
    return records_device_call(h, kCastTree, rays, ray_stride, ray_body, count, hits, hit_stride, caller_stream);
}

int tetsim_visual_bounding_spheres_device(tetsim_handle h, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    constexpr uint64_t row = 4ull * sizeof(double);
    if (int rc = check_record_stride(h, "row_stride", row_stride, row, 8u)) return rc;
    if (!dst) return fail(h, TETSIM_EINVAL, "dst is null");
    if (int rc = check_query_state(h, false)) return rc;
    if (int rc = device_call_guard(h)) return rc;
    const uint64_t stride = resolved_stride(row_stride, row);
    if (int rc = check_device_records(h, dst, stride, h->info.num_bodies, row, 8u, "dst")) return rc;
    return enqueue_query(h, QueryTables::kRows, Spheres::kBodies, caller_stream,
                         [&](const QueryDev&) { query_launch_spheres_out(h->stream, h->qbodies, static_cast<char*>(dst), stride); });
}

// ---- closest-point queries through the same tree (query_closest.hip); the definition: include/tetsim.h ------------------------------
int tetsim_closest_visual_device(tetsim_handle h, const void* queries, uint64_t query_stride, const void* query_body, uint32_t count, void* out,
                                 uint64_t out_stride, void* caller_stream) {
    return records_device_call(h, kClosestTree, queries, query_stride, query_body, count, out, out_stride, caller_stream);
}

// host arrays: staged through buffers that grow on demand, the same kernel, then a synchronisation; a query the host can see is bad is refused
int tetsim_closest_visual(tetsim_handle h, const TetSimPointQuery* queries, const int32_t* query_body, uint32_t count, TetSimClosest* out) {
    if (!h) return TETSIM_EINVAL;
    CastIo io;
    if (int rc = check_records(h, kQueries, queries, 0u, query_body, count, out, 0u, &io)) return rc;
    for (uint32_t i = 0; i < count; i++) {
        static const char* const why[] = {"", "non-finite point", "max_distance is NaN", "max_distance < 0"};
        if (const int defect = point_query_defect(queries[i].point, queries[i].max_distance)) return fail(h, TETSIM_EINVAL, "query " + std::to_string(i) + ": " + why[defect]);
        if (query_body && (query_body[i] < 0 || static_cast<uint32_t>(query_body[i]) >= h->info.num_bodies))
            return fail(h, TETSIM_EINVAL, "query " + std::to_string(i) + ": query_body is outside [0, num_bodies)");
    }
    if (count == 0) return 0;
    if (int rc = device_call_guard(h)) return rc;
    const size_t want = std::max<size_t>(count, 64);
    int rc;
    if ((rc = dev_grow(h, &h->d_point_queries, &h->point_query_cap, want)) || (rc = dev_grow(h, &h->d_closest, &h->closest_cap, want)) ||
        (query_body && (rc = dev_grow(h, &h->d_point_bodies, &h->point_body_cap, want)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (a previous call's kernel may still read the staging buffers)
    HIPCHK(h, hipMemcpy(h->d_point_queries, queries, count * sizeof(PointQueryIn), hipMemcpyHostToDevice));
    if (query_body) HIPCHK(h, hipMemcpy(h->d_point_bodies, query_body, count * sizeof(int32_t), hipMemcpyHostToDevice));
    io.in = reinterpret_cast<const char*>(h->d_point_queries);
    io.body = query_body ? h->d_point_bodies : nullptr;
    io.out = reinterpret_cast<char*>(h->d_closest);
    if ((rc = enqueue_records(h, kClosestTree, io, nullptr))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->d_closest, count * sizeof(ClosestOut), hipMemcpyDeviceToHost));
    return 0;
}

#ifdef TETSIM_BVH_STATS
// development builds only (tools/raycast_bvh_cost.py): the next tree casts count, per ray, the boxes and the triangles they test into
// stats [count][2] uint32 in DEVICE memory; NULL turns the counting off again
int tetsim_debug_bvh_stats(tetsim_handle h, void* stats) {
    if (!h) return TETSIM_EINVAL;
    h->bvh.stats = static_cast<uint32_t*>(stats);
    return 0;
}
// ... and the refit alone, with the call's handshake around it: no skinning, no spheres, no cast (the tree must exist)
int tetsim_debug_bvh_refit(tetsim_handle h, void* caller_stream) {
    if (!h || !h->bvh_ready) return TETSIM_EINVAL;
    return on_caller_stream(h, caller_stream, [&]() -> int {
        query_launch_bvh_refit(h->stream, query_view(h), h->qbodies, h->bvh);
        return launched(h);
    });
}
#endif

// The tree's topology without a device (query_device.h: bvh_build_topology, what the first tetsim_raycast_visual_bvh_device call builds from
// the positions of that moment).  positions [3 * nvis]; tri_ids [3 * ntri]; tri_body [ntri] or NULL (one body).  Out: tri_first [bodies + 1],
// order [ntri], node_first [bodies + 1], depth [bodies]; node_range, if not NULL, [node_first[bodies]][2]: the range in `order` of the
// triangles below every node (slot 0 of a body: 0, 0) -- call once with NULL to learn node_first[bodies].
int tetsim_prep_bvh(const float* positions, uint32_t nvis, const int32_t* tri_ids, uint32_t ntri, const int32_t* tri_body, uint32_t bodies,
                    uint32_t* tri_first, uint32_t* order, uint32_t* node_first, uint32_t* depth, uint32_t* node_range) {
    if ((nvis && !positions) || (ntri && !tri_ids) || bodies == 0 || !tri_first || (ntri && !order) || !node_first || !depth) return TETSIM_EINVAL;
    for (uint32_t t = 0; t < ntri; t++) {
        for (int k = 0; k < 3; k++)
            if (tri_ids[3 * static_cast<size_t>(t) + k] < 0 || static_cast<uint32_t>(tri_ids[3 * static_cast<size_t>(t) + k]) >= nvis) return TETSIM_EINVAL;
        if (tri_body && (tri_body[t] < 0 || static_cast<uint32_t>(tri_body[t]) >= bodies)) return TETSIM_EINVAL;
    }
    std::vector<uint32_t> first, sorted;
    sort_triangles_by_body(tri_body, ntri, bodies, &first, &sorted, nullptr);
    BvhTopology topo;
    if (!bvh_build_topology(positions, 3u, tri_ids, 3u, sorted.data(), first.data(), bodies, &topo).empty()) return TETSIM_EINVAL;
    std::copy(first.begin(), first.end(), tri_first);
    std::copy(topo.order.begin(), topo.order.end(), order);
    std::copy(topo.node_first.begin(), topo.node_first.end(), node_first);
    std::copy(topo.depth.begin(), topo.depth.end(), depth);
    if (node_range)
        for (uint32_t b = 0; b < bodies; b++) {
            const uint32_t n = first[b + 1u] - first[b], slots = 1u << topo.depth[b];
            uint32_t* const r = node_range + 2ull * topo.node_first[b];
            r[0] = r[1] = 0u;
            for (uint32_t i = 1; i < 2u * slots; i++) {
                uint32_t lo, hi;
                bvh_node_leaves(i, topo.depth[b], &lo, &hi);
                r[2ull * i] = first[b] + static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(lo) * kBvhLeaf, n));
                r[2ull * i + 1u] = first[b] + static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(hi) * kBvhLeaf, n));
            }
        }
    return 0;
}

}  // extern "C"
