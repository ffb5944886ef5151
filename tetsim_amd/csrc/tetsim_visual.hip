// tetsim_visual.hip -- C ABI, part 3 (include/tetsim.h): the embedded visual mesh (skinning, three.js computeVertexNormals; its rows
// leave through device_io.hip) and the grab interface (pin a particle; nearest-particle query on the device).  See body.h.
#include "body_rows.h"

using namespace tetsim;

extern "C" {

int tetsim_set_visual_mesh(tetsim_handle h, const float* vis_verts, uint32_t nvis, const float* rest_normals) {
    if (!h || (nvis && !vis_verts)) return fail(h, TETSIM_EINVAL, "null argument");
    if (h->vis_attached) return fail(h, TETSIM_ESTATE, "a visual mesh is already attached");
    HIPCHK(h, hipSetDevice(h->opt.device));
    const bool pjs = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI;
    const uint32_t nt = h->info.num_elems;
    // A PARTITION takes the same (global) list on every rank and keeps the visual vertices whose tet it OWNS by the lowest-owner rule
    // (TetSimInfo.owned_elems: every tet has exactly one such partition, and that partition solves it, so the tet's quaternion is
    // local); the union over the partitions is the whole visual mesh, tetsim_get_visual_ids says which rows a partition kept.
    // Corners of a kept tet are owned or ghost particles: the ghosts' end-of-substep positions are fetched by
    // tetsim_read_visual_mesh (tetsim_halo_refresh_final).
    std::vector<int32_t> g2l_tet, g2l_vert;
    if (h->partitioned) {
        g2l_tet.assign(nt, -1);
        for (size_t i = 0; i < h->part.local_to_global_tet.size(); i++) g2l_tet[h->part.local_to_global_tet[i]] = static_cast<int32_t>(i);
        g2l_vert.assign(h->info.num_particles, -1);
        for (size_t i = 0; i < h->part.local_to_global_vert.size(); i++) g2l_vert[h->part.local_to_global_vert[i]] = static_cast<int32_t>(i);
    }
    std::vector<int32_t> tet_pos;  // (local) tet id -> device tet position (quaternion index)
    if (pjs) {
        const uint32_t ntl = h->partitioned ? h->info.local_elems : nt;
        tet_pos.resize(ntl);
        for (uint32_t i = 0; i < ntl; i++) tet_pos[h->blocked ? h->tet_perm[i] : i] = static_cast<int32_t>(i);
    }
    std::vector<int4> corner;
    std::vector<float4> weight, n0;
    std::vector<uint32_t> vis_tet;
    std::vector<int32_t> qidx, kept, row_body;   // (row_body: batches -- moved into the handle only when the call has succeeded)
    for (uint32_t i = 0; i < nvis; i++) {
        const float tn = vis_verts[4 * i];
        if (!(tn >= 0.0f) || tn >= static_cast<float>(nt) || tn != std::floor(tn)) return fail(h, TETSIM_EINVAL, "visual vertex " + std::to_string(i) + " references a tet outside the mesh");
        const uint32_t e = static_cast<uint32_t>(tn);
        uint32_t el = e;   // the tet in this handle's numbering
        if (h->partitioned) {
            int lowest = h->opt.part_count;
            bool all_local = g2l_tet[e] >= 0;
            for (int k = 0; k < 4 && all_local; k++) {
                const int32_t lv = g2l_vert[h->h_tets[4 * e + k]];
                if (lv < 0) { all_local = false; break; }
                // owner of a local particle: this partition for the owned range, the neighbour whose receive range holds it otherwise
                int owner = h->opt.part_index;
                // (two-layer ghost regions keep the second layer in receive ranges of its own: a tet with such a corner belongs to the
                // neighbour too -- found in neither range it would pass for this partition's and be kept twice; advisor, round 5)
                if (static_cast<uint32_t>(lv) >= h->part.n_owned)
                    for (const auto& nb : h->part.neigh)
                        if ((static_cast<uint32_t>(lv) >= nb.recv_start && static_cast<uint32_t>(lv) < nb.recv_start + nb.recv_count) ||
                            (static_cast<uint32_t>(lv) >= nb.recv2_start && static_cast<uint32_t>(lv) < nb.recv2_start + nb.recv2_count)) owner = nb.rank;
                lowest = std::min(lowest, owner);
            }
            if (!all_local || lowest != h->opt.part_index) continue;   // another partition's row
            el = static_cast<uint32_t>(g2l_tet[e]);
        }
        int32_t c[4];
        for (int k = 0; k < 4; k++) {
            int32_t v = h->h_tets[4 * e + k];
            if (h->partitioned) v = g2l_vert[v];
            c[k] = (pjs && !h->api2dev.empty()) ? static_cast<int32_t>(h->api2dev[v]) : v;
        }
        corner.push_back(make_int4(c[0], c[1], c[2], c[3]));
        weight.push_back(make_float4(vis_verts[4 * i + 1], vis_verts[4 * i + 2], vis_verts[4 * i + 3], 0.0f));
        qidx.push_back(pjs ? tet_pos[el] : 0);
        if (rest_normals) n0.push_back(make_float4(rest_normals[3 * i], rest_normals[3 * i + 1], rest_normals[3 * i + 2], 0.0f));
        kept.push_back(static_cast<int32_t>(i));
        vis_tet.push_back(e);
        if (is_batch(h)) row_body.push_back(static_cast<int32_t>(body_of_tet(h, e)));   // (ray casts name the body of a hit: the body whose tets carry the row)
    }
    const uint32_t nk = static_cast<uint32_t>(kept.size());
    SkinDev& k = h->skin;
    int4* dc; float4 *dw, *dn = nullptr; int32_t* dq;
    int rc;
    if ((rc = dev_alloc(h, &dc, nk))) return rc;
    if ((rc = dev_alloc(h, &dw, nk))) return rc;
    if ((rc = dev_alloc(h, &dq, nk))) return rc;
    if ((rc = dev_alloc(h, &k.out_pos, nk))) return rc;
    if ((rc = upload(h, dc, corner))) return rc;
    if ((rc = upload(h, dw, weight))) return rc;
    if ((rc = upload(h, dq, qidx))) return rc;
    if (rest_normals && pjs) {
        if ((rc = dev_alloc(h, &dn, nk))) return rc;
        if ((rc = dev_alloc(h, &k.out_nrm, nk))) return rc;
        if ((rc = upload(h, dn, n0))) return rc;
    }
    k.corner = dc; k.weight = dw; k.qidx = dq; k.normal0 = dn;
    k.nvis = nk;
    h->vis_global = kept;
    h->vis_tet = vis_tet;
    h->vis_row_body = row_body;
    h->vis_total = nvis;
    h->vis_attached = true;
    h->info.num_vis_verts = nk;
    h->info.total_vis_verts = nvis;
    return 0;
}

int tetsim_get_visual_ids(tetsim_handle h, int32_t* out) {
    if (!h || !out) return fail(h, TETSIM_EINVAL, "null argument");
    if (!h->vis_attached) return fail(h, TETSIM_ESTATE, "no visual mesh attached (tetsim_set_visual_mesh)");
    std::copy(h->vis_global.begin(), h->vis_global.end(), out);
    return 0;
}

int tetsim_read_visual_mesh(tetsim_handle h, float* positions_out, float* normals_out) {
    if (!h || !positions_out) return fail(h, TETSIM_EINVAL, "null argument");
    const int32_t fields[2] = {TETSIM_FIELD_VISUAL_POSITIONS, TETSIM_FIELD_VISUAL_NORMALS};
    float* const out[2] = {positions_out, normals_out};
    const uint32_t count = normals_out ? 2u : 1u;
    FieldSrc f[2];
    std::string why;
    for (uint32_t k = 0; k < count; k++)
        if (int rc = resolve_field(h, fields[k], true, &f[k], &why)) return fail(h, rc, why);
    return read_fields(h, f, out, count);
}

int tetsim_set_visual_triangles(tetsim_handle h, const int32_t* tri_ids, uint32_t ntri) {
    if (!h || (ntri && !tri_ids)) return fail(h, TETSIM_EINVAL, "null argument");
    if (!h->vis_attached) return fail(h, TETSIM_ESTATE, "no visual mesh attached (tetsim_set_visual_mesh)");
    if (h->skin.vt_off) return fail(h, TETSIM_ESTATE, "visual triangles are already attached");
    HIPCHK(h, hipSetDevice(h->opt.device));
    // A PARTITION takes the same, global triangle list on every rank (ids = rows of the caller's visVerts) and keeps, for each row it
    // skins, that row's triangles in triangle order: a triangle's other corners may be skinned by other ranks, so the normals are computed
    // from the ranks' skins put together (tetsim_visual_vertex_normals_from) -- per vertex the same sums in the same order as unpartitioned.
    const bool part = h->partitioned;
    const uint32_t nrows = part ? h->vis_total : h->skin.nvis;      // what a triangle id may address
    const uint32_t nvis = h->skin.nvis;                              // the rows this handle computes normals for
    std::vector<int32_t> row_of;                                     // partitions: global row -> own row, or -1
    if (part) {
        row_of.assign(nrows, -1);
        for (uint32_t j = 0; j < nvis; j++) row_of[h->vis_global[j]] = static_cast<int32_t>(j);
    }
    auto own = [&](int32_t g) { return part ? row_of[g] : g; };
    std::vector<int4> tri(ntri);
    std::vector<uint32_t> off(nvis + 1, 0);
    for (uint32_t t = 0; t < ntri; t++) {
        for (int k = 0; k < 3; k++) {
            const int32_t v = tri_ids[3 * t + k];
            if (v < 0 || static_cast<uint32_t>(v) >= nrows) return fail(h, TETSIM_EINVAL, "triangle " + std::to_string(t) + " references a visual vertex outside the mesh");
            if (own(v) >= 0) off[own(v) + 1]++;
        }
        tri[t] = make_int4(tri_ids[3 * t], tri_ids[3 * t + 1], tri_ids[3 * t + 2], 0);
    }
    for (uint32_t v = 0; v < nvis; v++) off[v + 1] += off[v];
    std::vector<uint32_t> ent(off[nvis]), fill(off.begin(), off.end() - 1);
    for (uint32_t t = 0; t < ntri; t++)   // triangle order, corner order: the order of the reference's accumulation
        for (int k = 0; k < 3; k++) { const int32_t o = own(tri_ids[3 * t + k]); if (o >= 0) ent[fill[o]++] = t; }
    SkinDev& k = h->skin;
    int4* dt; uint32_t *doff, *dent;
    int rc;
    if ((rc = dev_alloc(h, &dt, ntri))) return rc;
    if ((rc = dev_alloc(h, &doff, off.size()))) return rc;
    if ((rc = dev_alloc(h, &dent, ent.size()))) return rc;
    if ((rc = dev_alloc(h, &k.out_vnrm, nvis))) return rc;
    if ((rc = dev_alloc(h, &h->d_vis_full, nrows))) return rc;   // (tetsim_visual_vertex_normals_from; unpartitioned bodies may use it too)
    if ((rc = upload(h, dt, tri))) return rc;
    if ((rc = upload(h, doff, off))) return rc;
    if ((rc = upload(h, dent, ent))) return rc;
    k.ntri = ntri; k.tri = dt; k.vt_tri = dent;
    if (!h->vis_row_body.empty() && !part) {
        h->tri_body.resize(ntri);
        for (uint32_t t = 0; t < ntri; t++) {
            h->tri_body[t] = h->vis_row_body[tri_ids[3 * t]];
            // (a per-body ray cast sees a body's own triangles: one that spans two bodies belongs to neither, tetsim_raycast_visual_device)
            if (h->vis_row_body[tri_ids[3 * t + 1]] != h->tri_body[t] || h->vis_row_body[tri_ids[3 * t + 2]] != h->tri_body[t]) h->tri_spans_bodies = true;
        }
    }
    k.vt_off = doff;
    return 0;
}

int tetsim_read_visual_vertex_normals(tetsim_handle h, float* normals_out) {
    if (!h || !normals_out) return fail(h, TETSIM_EINVAL, "null argument");
    FieldSrc f;
    std::string why;
    if (int rc = resolve_field(h, TETSIM_FIELD_VISUAL_VERTEX_NORMALS, true, &f, &why)) return fail(h, rc, why);
    if (h->partitioned) return fail(h, TETSIM_ESTATE, "a partition skins only its own rows, and a triangle's corners may belong to other ranks: put the ranks' skins together "
                                                      "(tetsim_read_visual_mesh + tetsim_get_visual_ids) and call tetsim_visual_vertex_normals_from, or tetsim_group_read_visual_vertex_normals");
    return read_fields(h, &f, &normals_out, 1);
}

// computeVertexNormals (Softbody.js:273) of THIS handle's rows from a complete set of visual positions -- for a partition the ranks'
// skins put together by the host (every rank's tetsim_read_visual_mesh scattered by tetsim_get_visual_ids), for an unpartitioned body
// any positions of its visual mesh.  Per vertex the face normals of its triangles are added in triangle order exactly as three.js
// does, so the partitions' rows equal the unpartitioned body's normals bit for bit.
int tetsim_visual_vertex_normals_from(tetsim_handle h, const float* all_positions, float* normals_out) {
    if (!h || !all_positions || !normals_out) return fail(h, TETSIM_EINVAL, "null argument");
    FieldSrc f;
    std::string why;
    if (int rc = resolve_field(h, TETSIM_FIELD_VISUAL_VERTEX_NORMALS, true, &f, &why)) return fail(h, rc, why);
    HIPCHK(h, hipSetDevice(h->opt.device));
    const uint32_t nrows = h->partitioned ? h->vis_total : h->skin.nvis;
    std::vector<float4> full(nrows);
    for (uint32_t i = 0; i < nrows; i++) full[i] = make_float4(all_positions[3 * i], all_positions[3 * i + 1], all_positions[3 * i + 2], 0.0f);
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (a previous call's kernel may still read the buffer)
    if (nrows) HIPCHK(h, hipMemcpy(h->d_vis_full, full.data(), nrows * sizeof(float4), hipMemcpyHostToDevice));
    SkinDev k = h->skin;
    k.tri_pos = h->d_vis_full;
    skin_launch_vertex_normals(h->stream, k);
    return read_rows(h, &f, &normals_out, 1);   // (the normals of THESE positions: nothing is skinned, so no prepare_fields)
}

// The partitions of ONE process: every member skins its rows (their ghosts' end-of-substep positions must be fresh:
// tetsim_group_refresh_final), the rows are put together, every member computes the normals of its rows from the whole.  positions_out /
// normals_out [3 * rows of visVerts], either may be NULL.  Equal to the unpartitioned body's tetsim_read_visual_mesh /
// tetsim_read_visual_vertex_normals bit for bit (PRECISE).
int tetsim_group_read_visual_vertex_normals(tetsim_handle* hs, uint32_t count, float* positions_out, float* normals_out) {
    group_begin(hs, count);
    auto impl = [&]() -> int {
        if (!hs || count == 0) return TETSIM_EINVAL;
        for (uint32_t i = 0; i < count; i++)
            if (!hs[i] || hs[i]->opt.part_count != static_cast<int32_t>(count) || hs[i]->opt.part_index != static_cast<int32_t>(i))
                return fail(hs[i], TETSIM_EINVAL, "handles[i] must be partition i of a count-way decomposition");
        const uint32_t total = hs[0]->vis_total;
        std::vector<float> full(3ull * total, 0.0f), rows, nrm;
        for (uint32_t i = 0; i < count; i++) {
            tetsim_body* h = hs[i];
            if (!h->vis_attached || h->vis_total != total) return fail(h, TETSIM_ESTATE, "every member needs the same visual mesh (tetsim_set_visual_mesh)");
            rows.resize(3ull * h->skin.nvis);
            if (int rc = tetsim_read_visual_mesh(h, rows.data(), nullptr)) return rc;
            for (uint32_t j = 0; j < h->skin.nvis; j++) std::memcpy(&full[3ull * h->vis_global[j]], &rows[3ull * j], 3 * sizeof(float));
        }
        if (positions_out) std::memcpy(positions_out, full.data(), full.size() * sizeof(float));
        if (!normals_out) return 0;
        for (uint32_t i = 0; i < count; i++) {
            tetsim_body* h = hs[i];
            nrm.resize(3ull * h->skin.nvis);
            if (int rc = tetsim_visual_vertex_normals_from(h, full.data(), nrm.data())) return rc;
            for (uint32_t j = 0; j < h->skin.nvis; j++) std::memcpy(&normals_out[3ull * h->vis_global[j]], &nrm[3ull * j], 3 * sizeof(float));
        }
        return 0;
    };
    return group_result(hs, count, impl());
}

int tetsim_set_grab(tetsim_handle h, int32_t id, const float xyz[3]) {
    if (!h) return TETSIM_EINVAL;
    if (id >= static_cast<int32_t>(h->info.num_particles)) return fail(h, TETSIM_EINVAL, "grab id out of range");
    if (id >= 0 && h->body_grabs_on) return fail(h, TETSIM_ESTATE, kBodyGrabsOn);   // (releasing the handle's grab, id < 0, stays legal)
    if (id >= 0 && h->body_pins_on) return fail(h, TETSIM_ESTATE, kBodyPinsOn);
    h->grab_global = id < 0 ? -1 : id;
    ref_grab_texels(h->grab_global, h->info.num_elems, h->info.num_particles, h->grab_ref);
    if (xyz) std::memcpy(h->grab_pos, xyz, 3 * sizeof(float));
    return 0;
}

// Kinematic colliders: checked and normalised in f64 as a whole (body_rows.h: collider_view, the routine the body colliders' set kernel
// runs per row), then they replace the list (a rejected call leaves the old one).
int tetsim_set_colliders(tetsim_handle h, const TetSimCollider* colliders, uint32_t count) {
    if (!h) return TETSIM_EINVAL;
    if (count > TETSIM_MAX_COLLIDERS) return fail(h, TETSIM_EINVAL, "more than TETSIM_MAX_COLLIDERS colliders");
    if (count && !colliders) return fail(h, TETSIM_EINVAL, "colliders is null");
    if (count && h->body_colliders_on) return fail(h, TETSIM_ESTATE, kBodyCollidersOn);   // (clearing the handle's list, count 0, stays legal)
    static const char* const kRefusal[] = {"unknown kind", "non-finite value", "negative radius or friction", "zero-length plane normal", "negative half-extent",
                                           "zero-length box axis", "box axes are not orthogonal"};
    DevColliderD d[kMaxColliders] = {};
    DevColliderF f[kMaxColliders] = {};
    for (uint32_t k = 0; k < count; k++) {
        const TetSimCollider& c = colliders[k];
        const std::string at = "collider " + std::to_string(k) + ": ";
        const int why = collider_view(static_cast<double>(c.kind), c.a, c.b, c.axes, c.radius, c.friction, c.velocity, &d[k]);
        if (why == kColliderKind) return fail(h, TETSIM_EINVAL, at + kRefusal[why - 1]);
        if (c.reserved != 0) return fail(h, TETSIM_EINVAL, at + "reserved must be 0");
        if (why != kColliderOk) return fail(h, TETSIM_EINVAL, at + kRefusal[why - 1]);
        f[k] = collider_f32(d[k]);
    }
    h->n_colliders = count;
    for (uint32_t k = 0; k < kMaxColliders; k++) { h->col[k] = f[k]; h->d_col[k] = d[k]; }
    return 0;
}

namespace {
// argmin of Softbody.js:279-291 over this handle's OWNED particles, on the device: one (d2, index) candidate per 256
// particles comes back.  *local receives the API-local index (first minimum), *best its squared distance (f64).
int nearest_owned(tetsim_body* h, const float xyz[3], int32_t* local, double* best_out) {
    HIPCHK(h, hipSetDevice(h->opt.device));
    const uint32_t n = h->info.owned_particles, nblk = (n + 255u) / 256u;
    int rc;
    if (!h->d_best) {
        if ((rc = dev_alloc(h, &h->d_best, nblk))) return rc;
        if ((rc = dev_alloc(h, &h->d_best_id, nblk))) return rc;
        if ((rc = ensure_index_map(h))) return rc;
    }
    if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
    util_launch_nearest(h->stream, current_positions(h), h->d_api2dev, n, static_cast<double>(xyz[0]), static_cast<double>(xyz[1]),
                        static_cast<double>(xyz[2]), h->d_best, h->d_best_id);
    std::vector<double> bd(nblk);
    std::vector<uint32_t> bi(nblk);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (nblk) {
        HIPCHK(h, hipMemcpy(bd.data(), h->d_best, nblk * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(bi.data(), h->d_best_id, nblk * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    double best = 1.7976931348623157e308;
    int32_t id = -1;
    for (uint32_t b = 0; b < nblk; b++)  // blocks are in ascending particle order: `<` keeps the first minimum
        if (bd[b] < best) { best = bd[b]; id = static_cast<int32_t>(bi[b]); }
    *local = id;
    *best_out = best;
    return 0;
}
}  // namespace

int tetsim_start_grab(tetsim_handle h, const float xyz[3], int32_t* id_out) {
    if (!h || !xyz) return fail(h, TETSIM_EINVAL, "null argument");
    if (h->body_grabs_on) return fail(h, TETSIM_ESTATE, kBodyGrabsOn);
    if (h->body_pins_on) return fail(h, TETSIM_ESTATE, kBodyPinsOn);
    if (h->partitioned) return fail(h, TETSIM_ESTATE, "start_grab on a partitioned body: combine tetsim_nearest_particle over the partitions on the host, then tetsim_set_grab on each");
    int32_t id = -1;
    double best = 0.0;
    int rc = nearest_owned(h, xyz, &id, &best);
    if (rc) return rc;
    h->grab_global = id;
    ref_grab_texels(h->grab_global, h->info.num_elems, h->info.num_particles, h->grab_ref);
    std::memcpy(h->grab_pos, xyz, 3 * sizeof(float));
    if (id_out) *id_out = id;
    return 0;
}

int tetsim_nearest_particle(tetsim_handle h, const float xyz[3], int32_t* global_id, double* dist2) {
    if (!h || !xyz || !global_id || !dist2) return fail(h, TETSIM_EINVAL, "null argument");
    int32_t local = -1;
    int rc = nearest_owned(h, xyz, &local, dist2);
    if (rc) return rc;
    *global_id = local < 0 ? -1 : (h->partitioned ? h->part.local_to_global_vert[local] : local);
    return 0;
}

// ---- picking: three.js r160 ray casts and the bounding sphere of the skinned visual mesh (query_kernels.hip) ----------------------
namespace {
static_assert(sizeof(TetSimRay) == sizeof(RayIn) && sizeof(TetSimRayHit) == sizeof(RayOut), "the ABI's ray records are the kernels' records");
const char* const kPartitionedQuery = "a partition skins only its own rows, and a triangle's corners may belong to other ranks: ray casts and the bounding sphere "
                                      "of a partitioned body are not supported (put the ranks' skins together with tetsim_read_visual_mesh + tetsim_get_visual_ids)";

// the visual positions of the last completed substep in skin.out_pos and their bounding sphere in d_sphere, on h->stream
int skin_for_query(tetsim_body* h, QueryDev* q);
int skin_and_sphere(tetsim_body* h, QueryDev* q) {
    HIPCHK(h, hipSetDevice(h->opt.device));
    if (int rc = skin_for_query(h, q)) return rc;
    query_launch_sphere(h->stream, *q);
    return 0;
}

int check_query_state(tetsim_body* h, bool need_triangles) {
    if (!h->vis_attached) return fail(h, TETSIM_ESTATE, "no visual mesh attached (tetsim_set_visual_mesh)");
    if (need_triangles && (!h->skin.vt_off || h->skin.ntri == 0)) return fail(h, TETSIM_ESTATE, "no visual triangles attached (tetsim_set_visual_triangles)");
    if (h->partitioned) return fail(h, TETSIM_ESTATE, kPartitionedQuery);
    if (h->skin.nvis == 0) return fail(h, TETSIM_ESTATE, "the visual mesh has no vertices");
    return 0;
}

int check_rays(tetsim_body* h, const TetSimRay* rays, uint32_t count) {
    for (uint32_t i = 0; i < count; i++) {
        // (ray_defect, query_device.h: the one definition of an invalid ray; the device's cast reads it too)
        static const char* const why[] = {"", "non-finite origin or direction", "zero direction", "near or far is NaN", "near < 0", "far < near"};
        const TetSimRay& r = rays[i];
        if (const int defect = ray_defect(r.origin, r.direction, r.near, r.far)) return fail(h, TETSIM_EINVAL, "ray " + std::to_string(i) + ": " + why[defect]);
    }
    return 0;
}

// the per-body tables of the visual rows (query_device.h), built and uploaded once: the body of every row, the rows of every body, the sphere keys
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

// ... and of the triangle list: the ids stably sorted by body with the bodies' offsets, the body of every triangle (batches), the candidates
// of the few-ray launches.  (A triangle whose rows belong to different bodies was found by tetsim_set_visual_triangles: tri_spans_bodies.)
int ensure_triangle_tables(tetsim_body* h) {
    if (h->qtris_ready) return 0;
    if (int rc = ensure_row_tables(h)) return rc;
    QueryBodiesDev& b = h->qbodies;
    const uint32_t nb = b.bodies, ntri = h->skin.ntri;
    auto body_of = [&](uint32_t t) { return h->tri_body.empty() ? 0u : static_cast<uint32_t>(h->tri_body[t]); };
    std::vector<uint32_t> first(nb + 1u, 0u), sorted(ntri);
    for (uint32_t t = 0; t < ntri; t++) first[body_of(t) + 1u]++;
    uint32_t most = 0;
    for (uint32_t k = 0; k < nb; k++) { most = std::max(most, first[k + 1u]); first[k + 1u] += first[k]; }
    std::vector<uint32_t> fill(first.begin(), first.end() - 1);
    for (uint32_t t = 0; t < ntri; t++) sorted[fill[body_of(t)]++] = t;   // (in list order: stable)
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

// skinning alone: the visual positions of the last enqueued substep in skin.out_pos, on h->stream
int skin_for_query(tetsim_body* h, QueryDev* q) {
    const bool pjs = h->opt.solver == TETSIM_SOLVER_POLAR_JACOBI;
    if (pjs) { if (int rc = ensure_quats(h)) return rc; }
    if (!h->d_sphere) { if (int rc = dev_alloc(h, &h->d_sphere, kSphereWords)) return rc; }
    skin_launch(h->stream, h->skin, pjs ? h->pj.pos_final : h->nh.pos, pjs ? h->pj.quat : nullptr, !pjs);
    q->nvis = h->skin.nvis; q->ntri = h->skin.ntri; q->pos = h->skin.out_pos; q->tri = h->skin.tri; q->sphere = h->d_sphere;
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
}  // namespace

int tetsim_raycast_visual(tetsim_handle h, const TetSimRay* rays, uint32_t count, TetSimRayHit* hits) {
    if (!h) return fail(h, TETSIM_EINVAL, "null argument");
    if (count && (!rays || !hits)) return fail(h, TETSIM_EINVAL, "null argument");
    if (int rc = check_query_state(h, true)) return rc;
    if (count == 0) return 0;
    return cast_rays(h, rays, count, hits);
}

int tetsim_start_grab_ray(tetsim_handle h, const TetSimRay* ray, TetSimRayHit* hit_out, int32_t* id_out) {
    if (!h || !ray) return fail(h, TETSIM_EINVAL, "null argument");
    if (h->body_grabs_on) return fail(h, TETSIM_ESTATE, kBodyGrabsOn);
    if (h->body_pins_on) return fail(h, TETSIM_ESTATE, kBodyPinsOn);
    if (int rc = check_query_state(h, true)) return rc;
    TetSimRayHit hit;
    if (int rc = cast_rays(h, ray, 1, &hit)) return rc;
    if (hit_out) *hit_out = hit;
    if (id_out) *id_out = -1;
    if (!hit.hit) return 0;   // (the grab stays as it was)
    // Grabber.start (Softbody.js:448-451): origin.clone().addScaledVector(direction, distance), handed to startGrab
    float xyz[3];
    for (int k = 0; k < 3; k++) xyz[k] = static_cast<float>(ray->origin[k] + ray->direction[k] * hit.distance);
    return tetsim_start_grab(h, xyz, id_out);
}

// ---- range sensors: the same casts and spheres per body, from and into the caller's device memory (query_device.h) -------------------
namespace {
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

// tetsim_raycast_visual_device and tetsim_raycast_visual_bvh_device: one signature, one list of errors, one handshake; `bvh` chooses the kernels
int raycast_device(tetsim_handle h, const void* rays, uint64_t ray_stride, const void* ray_body, uint32_t count, void* hits, uint64_t hit_stride,
                   void* caller_stream, bool bvh) {
    if (!h) return TETSIM_EINVAL;
    if (count && (!rays || !hits)) return fail(h, TETSIM_EINVAL, "null argument");
    constexpr uint64_t ray_row = sizeof(TetSimRay), hit_row = sizeof(TetSimRayHit);
    if (int rc = check_record_stride(h, "ray_stride", ray_stride, ray_row, 8u)) return rc;
    if (int rc = check_record_stride(h, "hit_stride", hit_stride, hit_row, 8u)) return rc;
    if (int rc = check_query_state(h, true)) return rc;
    if (ray_body && h->tri_spans_bodies)
        return fail(h, TETSIM_ESTATE, "a triangle of the visual mesh has rows of different bodies: it belongs to no body's own surface (cast without ray_body)");
    if (count == 0) return 0;
    if (int rc = device_call_guard(h)) return rc;
    CastIo io;
    io.rays = static_cast<const char*>(rays); io.ray_stride = ray_stride ? ray_stride : ray_row;
    io.ray_body = static_cast<const int32_t*>(ray_body);
    io.hits = static_cast<char*>(hits); io.hit_stride = hit_stride ? hit_stride : hit_row;
    io.count = count;
    if (int rc = check_device_records(h, rays, io.ray_stride, count, ray_row, 8u, "rays")) return rc;
    if (int rc = check_device_records(h, hits, io.hit_stride, count, hit_row, 8u, "hits")) return rc;
    if (ray_body) { if (int rc = check_device_records(h, ray_body, 4u, count, 4u, 4u, "ray_body")) return rc; }
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    if (int rc = ensure_triangle_tables(h)) return rc;
    if (bvh) { if (int rc = ensure_bvh(h)) return rc; }
    return on_caller_stream(h, caller_stream, [&]() -> int {
        QueryDev q;
        if (int rc = skin_for_query(h, &q)) return rc;
        if (ray_body) query_launch_body_spheres(h->stream, q, h->qbodies);
        else query_launch_sphere(h->stream, q);
        if (bvh) {
            query_launch_bvh_refit(h->stream, q, h->qbodies, h->bvh);
            query_launch_cast_bvh(h->stream, q, h->qbodies, h->bvh, io);
        } else {
            query_launch_cast_device(h->stream, q, h->qbodies, io, h->d_cast_cand);
        }
        return launched(h);
    });
}
}  // namespace

int tetsim_raycast_visual_device(tetsim_handle h, const void* rays, uint64_t ray_stride, const void* ray_body, uint32_t count, void* hits, uint64_t hit_stride,
                                 void* caller_stream) {
    return raycast_device(h, rays, ray_stride, ray_body, count, hits, hit_stride, caller_stream, false);
}

// the same casts through the refitted tree (query_bvh.hip); its own definition: include/tetsim.h
int tetsim_raycast_visual_bvh_device(tetsim_handle h, const void* rays, uint64_t ray_stride, const void* ray_body, uint32_t count, void* hits,
                                     uint64_t hit_stride, void* caller_stream) {
    return raycast_device(h, rays, ray_stride, ray_body, count, hits, hit_stride, caller_stream, true);
}

// ---- closest-point queries through the same tree (query_closest.hip); the definition: include/tetsim.h ------------------------------
namespace {
static_assert(sizeof(TetSimPointQuery) == sizeof(PointQueryIn) && sizeof(TetSimClosest) == sizeof(ClosestOut), "the ABI's query records are the kernel's records");

// what tetsim_closest_visual_device checks before it enqueues anything, the list of tetsim_raycast_visual_bvh_device; *io: the resolved records
int closest_check(tetsim_handle h, const void* queries, uint64_t query_stride, const void* query_body, uint32_t count, void* out, uint64_t out_stride, ClosestIo* io) {
    if (count && (!queries || !out)) return fail(h, TETSIM_EINVAL, "null argument");
    constexpr uint64_t query_row = sizeof(TetSimPointQuery), out_row = sizeof(TetSimClosest);
    if (int rc = check_record_stride(h, "query_stride", query_stride, query_row, 8u)) return rc;
    if (int rc = check_record_stride(h, "out_stride", out_stride, out_row, 8u)) return rc;
    if (int rc = check_query_state(h, true)) return rc;
    if (query_body && h->tri_spans_bodies)
        return fail(h, TETSIM_ESTATE, "a triangle of the visual mesh has rows of different bodies: it belongs to no body's own surface (query without query_body)");
    io->queries = static_cast<const char*>(queries); io->query_stride = query_stride ? query_stride : query_row;
    io->query_body = static_cast<const int32_t*>(query_body);
    io->out = static_cast<char*>(out); io->out_stride = out_stride ? out_stride : out_row;
    io->count = count;
    return 0;
}

// behind the checks: the tables and the tree (only a handle's first tree call blocks), then skinning, spheres, refit and the queries on the handle's stream
int closest_enqueue(tetsim_handle h, const ClosestIo& io, void* caller_stream) {
    if (int rc = ensure_triangle_tables(h)) return rc;
    if (int rc = ensure_bvh(h)) return rc;
    return on_caller_stream(h, caller_stream, [&]() -> int {
        QueryDev q;
        if (int rc = skin_for_query(h, &q)) return rc;
        if (io.query_body) query_launch_body_spheres(h->stream, q, h->qbodies);
        else query_launch_sphere(h->stream, q);
        query_launch_bvh_refit(h->stream, q, h->qbodies, h->bvh);
        query_launch_closest_bvh(h->stream, q, h->qbodies, h->bvh, io);
        return launched(h);
    });
}
}  // namespace

int tetsim_closest_visual_device(tetsim_handle h, const void* queries, uint64_t query_stride, const void* query_body, uint32_t count, void* out,
                                 uint64_t out_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    ClosestIo io;
    if (int rc = closest_check(h, queries, query_stride, query_body, count, out, out_stride, &io)) return rc;
    if (count == 0) return 0;
    if (int rc = device_call_guard(h)) return rc;
    if (int rc = check_device_records(h, queries, io.query_stride, count, sizeof(TetSimPointQuery), 8u, "queries")) return rc;
    if (int rc = check_device_records(h, out, io.out_stride, count, sizeof(TetSimClosest), 8u, "out")) return rc;
    if (query_body) { if (int rc = check_device_records(h, query_body, 4u, count, 4u, 4u, "query_body")) return rc; }
    // ---- every argument is good: from here on only allocation and HIP itself can fail
    return closest_enqueue(h, io, caller_stream);
}

// host arrays: staged through buffers that grow on demand, the same kernel, then a synchronisation; a query the host can see is bad is refused
int tetsim_closest_visual(tetsim_handle h, const TetSimPointQuery* queries, const int32_t* query_body, uint32_t count, TetSimClosest* out) {
    if (!h) return TETSIM_EINVAL;
    ClosestIo io;
    if (int rc = closest_check(h, queries, 0u, query_body, count, out, 0u, &io)) return rc;
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
    io.queries = reinterpret_cast<const char*>(h->d_point_queries);
    io.query_body = query_body ? h->d_point_bodies : nullptr;
    io.out = reinterpret_cast<char*>(h->d_closest);
    if ((rc = closest_enqueue(h, io, nullptr))) return rc;
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
        QueryDev q;
        q.nvis = h->skin.nvis; q.ntri = h->skin.ntri; q.pos = h->skin.out_pos; q.tri = h->skin.tri; q.sphere = h->d_sphere;
        query_launch_bvh_refit(h->stream, q, h->qbodies, h->bvh);
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
    std::vector<uint32_t> first(bodies + 1u, 0u), sorted(ntri);
    for (uint32_t t = 0; t < ntri; t++) first[(tri_body ? tri_body[t] : 0) + 1u]++;
    for (uint32_t k = 0; k < bodies; k++) first[k + 1u] += first[k];
    std::vector<uint32_t> fill(first.begin(), first.end() - 1);
    for (uint32_t t = 0; t < ntri; t++) sorted[fill[tri_body ? tri_body[t] : 0]++] = t;
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

int tetsim_visual_bounding_spheres_device(tetsim_handle h, void* dst, uint64_t row_stride, void* caller_stream) {
    if (!h) return TETSIM_EINVAL;
    constexpr uint64_t row = 4ull * sizeof(double);
    if (int rc = check_record_stride(h, "row_stride", row_stride, row, 8u)) return rc;
    if (!dst) return fail(h, TETSIM_EINVAL, "dst is null");
    if (int rc = check_query_state(h, false)) return rc;
    if (int rc = device_call_guard(h)) return rc;
    const uint64_t stride = row_stride ? row_stride : row;
    if (int rc = check_device_records(h, dst, stride, h->info.num_bodies, row, 8u, "dst")) return rc;
    if (int rc = ensure_row_tables(h)) return rc;
    return on_caller_stream(h, caller_stream, [&]() -> int {
        QueryDev q;
        if (int rc = skin_for_query(h, &q)) return rc;
        query_launch_body_spheres(h->stream, q, h->qbodies);
        query_launch_spheres_out(h->stream, h->qbodies, static_cast<char*>(dst), stride);
        return launched(h);
    });
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

}  // extern "C"
