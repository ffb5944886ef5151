// tetsim_visual.hip -- C ABI, part 3 (include/tetsim.h): the embedded visual mesh (skinning, three.js computeVertexNormals; its rows
// leave through device_io.hip), the grab interface (pin a particle; nearest-particle query on the device; the grab along a ray) and the
// handle's kinematic colliders.  Queries on the visual mesh: tetsim_query.hip.  See body.h.
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

namespace {
// the handle's grab is refused while the bodies have grabs or pins of their own
int handle_grab_refused(tetsim_body* h) {
    if (h->body_grabs_on) return fail(h, TETSIM_ESTATE, kBodyGrabsOn);
    if (h->body_pins_on) return fail(h, TETSIM_ESTATE, kBodyPinsOn);
    return 0;
}
}  // namespace

int tetsim_set_grab(tetsim_handle h, int32_t id, const float xyz[3]) {
    if (!h) return TETSIM_EINVAL;
    if (id >= static_cast<int32_t>(h->info.num_particles)) return fail(h, TETSIM_EINVAL, "grab id out of range");
    if (id >= 0) { if (int rc = handle_grab_refused(h)) return rc; }   // (releasing the handle's grab, id < 0, stays legal)
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
    if (int rc = handle_grab_refused(h)) return rc;
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

int tetsim_start_grab_ray(tetsim_handle h, const TetSimRay* ray, TetSimRayHit* hit_out, int32_t* id_out) {
    if (!h || !ray) return fail(h, TETSIM_EINVAL, "null argument");
    if (int rc = handle_grab_refused(h)) return rc;
    TetSimRayHit hit;
    if (int rc = tetsim_raycast_visual(h, ray, 1, &hit)) return rc;   // (tetsim_query.hip: the query's state, the ray, the cast)
    if (hit_out) *hit_out = hit;
    if (id_out) *id_out = -1;
    if (!hit.hit) return 0;   // (the grab stays as it was)
    // Grabber.start (Softbody.js:448-451): origin.clone().addScaledVector(direction, distance), handed to startGrab
    float xyz[3];
    for (int k = 0; k < 3; k++) xyz[k] = static_cast<float>(ray->origin[k] + ray->direction[k] * hit.distance);
    return tetsim_start_grab(h, xyz, id_out);
}

}  // extern "C"
