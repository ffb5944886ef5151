// tetsim_host.cpp -- entry points that never touch a device: preprocessing, partition plans, the .tetsim container.
#include "body_rows.h"

using namespace tetsim;

namespace tetsim {
// The strain calls' constant record of every tet (strain.hip): the caller's corner ids, the f32 invRestPose of prep_rest, |V0| of the
// observation's rest volume, and the mark of a tet without a usable rest shape.
void build_strain_table(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, double density, StrainRec* out) {
    std::vector<float> inv_mass(nv), irp(9ull * nt), irv(nt);
    prep_rest(verts, nv, tets, nt, density, inv_mass.data(), irp.data(), irv.data());
    for (uint32_t e = 0; e < nt; e++) {
        StrainRec& r = out[e];
        const int32_t* t = &tets[4ull * e];
        const double v0 = rest_volume(verts, t);
        bool finite = true;
        for (uint32_t k = 0; k < 9u; k++) {
            r.b[k] = irp[9ull * e + k];
            finite = finite && std::isfinite(r.b[k]);
        }
        for (uint32_t k = 0; k < 4u; k++) r.id[k] = t[k];
        r.degenerate = (v0 == 0.0 || !finite) ? 1u : 0u;
        r.v0_abs = std::fabs(v0);
    }
}
// The pose calls' constant record of every particle (pose.hip; include/tetsim.h, THE TABLE): the lumped mass of the observation's w, corner
// by corner in tet order, and the rest position relative to its body's rest mass centre.  f64, every operation rounded on its own.
void build_pose_table(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, const uint32_t* first_vert, uint32_t bodies, double density,
                      PoseRec* out, double* centres) {
    for (uint32_t i = 0; i < nv; i++) out[i].m = 0.0;
    for (uint32_t e = 0; e < nt; e++) {
        const int32_t* t = &tets[4ull * e];
        const double w = (density * rest_volume(verts, t)) / 4.0;
        for (uint32_t k = 0; k < 4u; k++) out[t[k]].m = out[t[k]].m + w;
    }
    for (uint32_t b = 0; b < bodies; b++) {
        double m0 = 0.0, s[3] = {0.0, 0.0, 0.0}, c0[3] = {0.0, 0.0, 0.0};
        for (uint32_t i = first_vert[b]; i < first_vert[b + 1]; i++) {
            m0 = m0 + out[i].m;
            for (uint32_t k = 0; k < 3u; k++) s[k] = s[k] + out[i].m * static_cast<double>(verts[3ull * i + k]);
        }
        if (m0 != 0.0)
            for (uint32_t k = 0; k < 3u; k++) c0[k] = s[k] / m0;
        for (uint32_t i = first_vert[b]; i < first_vert[b + 1]; i++)
            for (uint32_t k = 0; k < 3u; k++) out[i].q[k] = static_cast<double>(verts[3ull * i + k]) - c0[k];
        if (centres)
            for (uint32_t k = 0; k < 3u; k++) centres[3ull * b + k] = c0[k];
    }
}
}  // namespace tetsim

extern "C" {

// ---- .tetsim mesh container ---------------------------------------------------------------------------------------
struct tetsim_mesh_file { tetsim::MeshFile* m; };

int tetsim_mesh_write(const char* path, const TetSimMeshArrays* a) {
    if (!a) return fail(nullptr, TETSIM_EINVAL, "arrays is null");
    const std::string e = mesh_write(path, *a);
    return e.empty() ? TETSIM_OK : fail(nullptr, TETSIM_EINVAL, e);
}
int tetsim_mesh_open(const char* path, tetsim_mesh* out) {
    if (!out) return fail(nullptr, TETSIM_EINVAL, "out is null");
    *out = nullptr;
    tetsim::MeshFile* m = nullptr;
    const std::string e = mesh_open(path, &m);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    *out = new tetsim_mesh_file{m};
    return TETSIM_OK;
}
int tetsim_mesh_arrays(tetsim_mesh m, TetSimMeshArrays* out) {
    if (!m || !out) return fail(nullptr, TETSIM_EINVAL, "null argument");
    *out = mesh_arrays(m->m);
    return TETSIM_OK;
}
int tetsim_mesh_close(tetsim_mesh m) {
    if (!m) return TETSIM_OK;
    mesh_close(m->m);
    delete m;
    return TETSIM_OK;
}

// ---- host-only preprocessing ---------------------------------------------------------------------------------
int tetsim_prep_levels(const int32_t* tets, uint32_t nt, uint32_t nv, int32_t* level, uint32_t* num_levels) {
    if ((nt && (!tets || !level)) || !num_levels) return TETSIM_EINVAL;
    std::string e = validate_mesh(reinterpret_cast<const float*>(tets), nv ? nv : 1, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    *num_levels = prep_levels(tets, nt, nv, level);
    return 0;
}
int tetsim_prep_colours(const int32_t* tets, uint32_t nt, uint32_t nv, int32_t* colour, uint32_t* num_colours) {
    if ((nt && (!tets || !colour)) || !num_colours) return TETSIM_EINVAL;
    std::string e = validate_mesh(reinterpret_cast<const float*>(tets), nv ? nv : 1, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    *num_colours = prep_colours(tets, nt, nv, colour);
    return 0;
}
int tetsim_prep_clusters(const int32_t* tets, uint32_t nt, uint32_t nv, int32_t* order, int32_t* launch, int32_t* lane, int32_t* step,
                         uint32_t* num_launches, uint32_t* num_clusters) {
    if ((nt && (!tets || !order || !launch || !lane || !step)) || !num_launches) return TETSIM_EINVAL;
    std::string e = validate_mesh(reinterpret_cast<const float*>(tets), nv ? nv : 1, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    const ClusterPlan P = prep_clusters(tets, nt, nv);
    for (uint32_t i = 0; i < nt; i++) order[i] = P.pre[i];
    const uint32_t nl = static_cast<uint32_t>(P.launch_off.size() - 1);
    for (uint32_t l = 0; l < nl; l++)
        for (uint32_t j = P.step_off[l]; j < P.step_off[l + 1]; j++)
            for (uint32_t i = 0; i < P.step_count[j]; i++) {
                const uint32_t pos = P.exec_pos[P.step_first[j] + i];
                launch[pos] = static_cast<int32_t>(l);
                lane[pos] = static_cast<int32_t>(i);
                step[pos] = static_cast<int32_t>(j - P.step_off[l]);
            }
    *num_launches = nl;
    if (num_clusters) *num_clusters = P.num_clusters;
    return 0;
}
int tetsim_prep_tiles(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, const uint32_t* body_first_tet,
                      const uint32_t* body_first_vert, uint32_t bodies, int32_t* tile_tets, uint32_t* tile_off, uint8_t* corner_slot,
                      uint32_t* num_tiles) {
    if (!num_tiles) return TETSIM_EINVAL;
    std::string e = validate_mesh(verts, nv, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    if (body_first_tet && body_first_vert && bodies) {
        if (body_first_tet[0] != 0 || body_first_vert[0] != 0 || body_first_tet[bodies] != nt || body_first_vert[bodies] != nv)
            return fail(nullptr, TETSIM_EINVAL, "body ranges must cover the whole mesh");
        for (uint32_t b = 0; b < bodies; b++) {
            if (body_first_tet[b] > body_first_tet[b + 1] || body_first_vert[b] >= body_first_vert[b + 1]) return fail(nullptr, TETSIM_EINVAL, "body ranges must ascend");
            for (uint64_t i = 4ull * body_first_tet[b]; i < 4ull * body_first_tet[b + 1]; i++)
                if (static_cast<uint32_t>(tets[i]) < body_first_vert[b] || static_cast<uint32_t>(tets[i]) >= body_first_vert[b + 1])
                    return fail(nullptr, TETSIM_EINVAL, "a tet references a particle of another body");
        }
    }
    const Incidence inc = build_incidence(tets, nt, nv, false, false);
    BlockPlan B;
    build_blocks(verts, tets, nt, nv, nv, inc, &B, body_first_tet, body_first_vert, bodies);
    *num_tiles = B.num_blocks;
    if (tile_tets) std::copy(B.tet_perm.begin(), B.tet_perm.end(), tile_tets);
    if (tile_off) std::copy(B.blk_tet_off.begin(), B.blk_tet_off.end(), tile_off);
    if (corner_slot) std::copy(B.tet_lidx.begin(), B.tet_lidx.end(), corner_slot);
    return 0;
}
int tetsim_prep_tile_tables(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, int32_t ref_table, uint32_t sizes[2], int32_t* tile_tets,
                            uint32_t* tile_off, uint32_t* slot_off, int32_t* slot_particle, uint8_t* corner_slot, uint16_t* entries, uint32_t* ranges,
                            uint32_t* tet_pos, uint16_t* run_first) {
    if (!sizes) return TETSIM_EINVAL;
    std::string e = validate_mesh(verts, nv, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    const Incidence inc = build_incidence(tets, nt, nv, ref_table != 0, ref_table != 0);
    BlockPlan B;
    build_blocks(verts, tets, nt, nv, nv, inc, &B);
    sizes[0] = B.num_blocks; sizes[1] = static_cast<uint32_t>(B.blk_verts.size());
    if (tile_tets) std::copy(B.tet_perm.begin(), B.tet_perm.end(), tile_tets);
    if (tile_off) std::copy(B.blk_tet_off.begin(), B.blk_tet_off.end(), tile_off);
    if (slot_off) std::copy(B.blk_vert_off.begin(), B.blk_vert_off.end(), slot_off);
    if (slot_particle) std::copy(B.blk_verts.begin(), B.blk_verts.end(), slot_particle);
    if (corner_slot) std::copy(B.tet_lidx.begin(), B.tet_lidx.end(), corner_slot);
    if (entries) std::copy(B.lc_ent.begin(), B.lc_ent.end(), entries);
    if (ranges) std::copy(B.lc_range.begin(), B.lc_range.end(), ranges);
    if (tet_pos) std::copy(B.tet_pos.begin(), B.tet_pos.end(), tet_pos);
    if (run_first) std::copy(B.lc_first.begin(), B.lc_first.end(), run_first);
    return 0;
}
int tetsim_prep_collider_views(const TetSimCollider* colliders, uint32_t count, int32_t as_rows, int32_t* codes, void* views_f64, void* views_f32) {
    if ((count && !colliders) || !codes || !views_f64 || !views_f32) return TETSIM_EINVAL;
    static_assert(sizeof(DevColliderD) == TETSIM_COLLIDER_VIEW_F64_BYTES && sizeof(DevColliderF) == TETSIM_COLLIDER_VIEW_F32_BYTES, "the views' sizes are in the header");
    for (uint32_t k = 0; k < count; k++) {
        const TetSimCollider& c = colliders[k];
        DevColliderD d;
        DevColliderF f;
        std::memset(&d, 0, sizeof d);
        std::memset(&f, 0, sizeof f);
        if (as_rows) {   // the collider as a row of tetsim_set_body_colliders holds it: every field an f32
            float r[21] = {static_cast<float>(c.kind)};
            for (int j = 0; j < 3; j++) { r[1 + j] = static_cast<float>(c.a[j]); r[4 + j] = static_cast<float>(c.b[j]); r[18 + j] = static_cast<float>(c.velocity[j]); }
            for (int j = 0; j < 9; j++) r[7 + j] = static_cast<float>(c.axes[j]);
            r[16] = static_cast<float>(c.radius); r[17] = static_cast<float>(c.friction);
            codes[k] = collider_view(r[0], r + 1, r + 4, r + 7, r[16], r[17], r + 18, &d);
        } else codes[k] = collider_view(static_cast<double>(c.kind), c.a, c.b, c.axes, c.radius, c.friction, c.velocity, &d);
        if (codes[k] == kColliderOk) f = collider_f32(d);
        else std::memset(&d, 0, sizeof d);
        std::memcpy(static_cast<char*>(views_f64) + static_cast<size_t>(k) * sizeof d, &d, sizeof d);
        std::memcpy(static_cast<char*>(views_f32) + static_cast<size_t>(k) * sizeof f, &f, sizeof f);
    }
    return 0;
}
int tetsim_prep_slot_table(const int32_t* tets, uint32_t nt, uint32_t nv, int32_t ref_quirk, int32_t* slots, uint32_t* dropped) {
    if ((nt && !tets) || !slots) return TETSIM_EINVAL;
    std::string e = validate_mesh(reinterpret_cast<const float*>(tets), nv ? nv : 1, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    const uint32_t d = prep_slot_table(tets, nt, nv, ref_quirk != 0, slots);
    if (dropped) *dropped = d;
    return 0;
}
int tetsim_prep_call_tiles(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, uint32_t sizes[4], uint32_t* blk_vert_off,
                           int32_t* blk_verts, uint32_t* vp_ell) {
    if (!sizes) return TETSIM_EINVAL;
    std::string e = validate_mesh(verts, nv, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    // particles in the device's numbering (tetsim_create: along a Morton curve), tiles as an unpartitioned body gets them
    const std::vector<uint32_t> order = morton_vertex_order(verts, nv, 0, nv);
    std::vector<int32_t> to_dev(nv), ltets(4ull * nt);
    std::vector<float> lverts(3ull * nv);
    for (uint32_t i = 0; i < nv; i++) {
        to_dev[order[i]] = static_cast<int32_t>(i);
        for (int c = 0; c < 3; c++) lverts[3ull * i + c] = verts[3ull * order[i] + c];
    }
    for (uint64_t i = 0; i < 4ull * nt; i++) ltets[i] = to_dev[tets[i]];
    const Incidence inc = build_incidence(ltets.data(), nt, nv, false, false);
    BlockPlan B;
    build_blocks(lverts.data(), ltets.data(), nt, nv, nv, inc, &B);
    sizes[0] = B.num_blocks; sizes[1] = static_cast<uint32_t>(B.blk_verts.size()); sizes[2] = B.vp_cols; sizes[3] = B.nv_pad;
    if (blk_vert_off) std::copy(B.blk_vert_off.begin(), B.blk_vert_off.end(), blk_vert_off);
    if (blk_verts) std::copy(B.blk_verts.begin(), B.blk_verts.end(), blk_verts);
    if (vp_ell) std::copy(B.vp_ell.begin(), B.vp_ell.begin() + static_cast<std::ptrdiff_t>(static_cast<size_t>(B.vp_cols) * B.nv_pad), vp_ell);
    return 0;
}
int tetsim_prep_call_schedule(const int32_t* blk_verts, const uint32_t* blk_vert_off, uint32_t nb, const uint32_t* vp_ell, uint32_t vp_cols,
                              uint32_t nv_pad, uint32_t nv_owned, uint32_t lag, uint32_t* entry, uint32_t capacity, uint32_t* period,
                              uint32_t* tail, int32_t* fell_back) {
    if (!blk_vert_off || (nb && !blk_verts) || (vp_cols && !vp_ell) || !period || !tail) return TETSIM_EINVAL;
    if (nv_owned > nv_pad && vp_cols) return fail(nullptr, TETSIM_EINVAL, "tetsim_prep_call_schedule: nv_owned exceeds the column stride of vp_ell");
    CallSchedule S;
    build_call_schedule(blk_verts, blk_vert_off, nb, vp_ell, vp_cols, nv_pad, nv_owned, lag, &S);
    *period = S.period; *tail = S.tail;
    if (fell_back) *fell_back = S.fell_back ? 1 : 0;
    if (S.fell_back) fail(nullptr, TETSIM_OK, "tetsim_prep_call_schedule: " + S.why + " -- the plain order instead");   // (reported, not an error: tetsim_last_error)
    if (entry) {
        if (capacity < S.period) return fail(nullptr, TETSIM_EINVAL, "tetsim_prep_call_schedule: the table needs " + std::to_string(S.period) + " entries");
        std::copy(S.entry.begin(), S.entry.end(), entry);
    }
    return 0;
}
int tetsim_prep_check_call_schedule(const int32_t* blk_verts, const uint32_t* blk_vert_off, uint32_t nb, const uint32_t* vp_ell, uint32_t vp_cols,
                                    uint32_t nv_pad, uint32_t nv_owned, const uint32_t* entry, uint32_t period, uint32_t tail) {
    if (!blk_vert_off || (nb && !blk_verts) || (vp_cols && !vp_ell) || !entry) return TETSIM_EINVAL;
    const std::string bad = check_call_schedule(blk_verts, blk_vert_off, nb, vp_ell, vp_cols, nv_pad, nv_owned, entry, period, tail);
    return bad.empty() ? 0 : fail(nullptr, TETSIM_EINVAL, "call schedule: " + bad);
}
int tetsim_prep_ref_grab_texels(int32_t grab_id, uint32_t num_elems, uint32_t num_particles, int32_t out[2]) {
    if (!out) return TETSIM_EINVAL;
    ref_grab_texels(grab_id, num_elems, num_particles, out);
    return 0;
}
// The pin table's normalisation (include/tetsim.h: tetsim_set_body_pins), the host's statement of what body_pins.hip's kernels do: rows in
// ascending order, so the first valid row to name a particle keeps it -- the integer minimum the device takes.
int tetsim_prep_pin_slots(const int32_t* particles, const float* targets, uint32_t num_bodies, uint32_t per_body, const uint32_t* body_particles, int32_t* slot_out) {
    if (!particles || !targets || !body_particles || !slot_out || per_body == 0u) return TETSIM_EINVAL;
    if (static_cast<uint64_t>(per_body) * num_bodies >= 0x80000000ull) return TETSIM_EINVAL;
    size_t first = 0;
    for (uint32_t b = 0; b < num_bodies; b++) {
        const uint32_t n = body_particles[b];
        int32_t* const slot = slot_out + first;
        for (uint32_t i = 0; i < n; i++) slot[i] = -1;
        for (uint32_t k = 0; k < per_body; k++) {
            const size_t row = static_cast<size_t>(b) * per_body + k;
            const int32_t p = particles[row];
            const float* const t = targets + 3u * row;
            if (p < 0 || static_cast<uint32_t>(p) >= n) continue;
            if (!finite_value(t[0]) || !finite_value(t[1]) || !finite_value(t[2])) continue;
            if (slot[p] < 0) slot[p] = static_cast<int32_t>(row);
        }
        first += n;
    }
    return 0;
}
int tetsim_prep_boundary_surface(const float* verts, const int32_t* tets, uint32_t nt, uint32_t nv, float* vis_verts, int32_t* tri_ids,
                                 uint32_t* nrows, uint32_t* ntri) {
    if ((nt && !tets) || !nrows || !ntri || (!vis_verts != !tri_ids)) return fail(nullptr, TETSIM_EINVAL, "tetsim_prep_boundary_surface: null argument");
    if (nt && nv == 0) return fail(nullptr, TETSIM_EINVAL, "tetsim_prep_boundary_surface: tets without particles (nv == 0)");
    std::string e = validate_mesh(reinterpret_cast<const float*>(tets), nv ? nv : 1, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    if (nt > (1u << 24)) return fail(nullptr, TETSIM_EINVAL, "tetsim_prep_boundary_surface: a tet id above 2^24 does not fit the f32 row format");
    // face k lies opposite corner k; for a positively oriented tet these windings look counter-clockwise from outside
    static const int kFace[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};
    struct Face { int32_t key[3]; uint32_t tet, face; };
    std::vector<Face> faces(4ull * nt);
    for (uint32_t t = 0; t < nt; t++)
        for (uint32_t k = 0; k < 4; k++) {
            Face& f = faces[4ull * t + k];
            for (int j = 0; j < 3; j++) f.key[j] = tets[4 * t + kFace[k][j]];
            std::sort(f.key, f.key + 3);
            f.tet = t; f.face = k;
        }
    std::sort(faces.begin(), faces.end(), [](const Face& a, const Face& b) {
        return std::lexicographical_compare(a.key, a.key + 3, b.key, b.key + 3) || (std::equal(a.key, a.key + 3, b.key) && (a.tet < b.tet || (a.tet == b.tet && a.face < b.face)));
    });
    std::vector<uint64_t> boundary;   // 4 * tet + face, ascending
    for (size_t i = 0; i < faces.size();) {
        size_t j = i + 1;
        while (j < faces.size() && std::equal(faces[i].key, faces[i].key + 3, faces[j].key)) j++;
        if (j - i == 1) boundary.push_back(4ull * faces[i].tet + faces[i].face);
        i = j;
    }
    std::sort(boundary.begin(), boundary.end());
    std::vector<int32_t> row(nv, -1);   // particle -> row
    for (uint64_t b : boundary)
        for (int j = 0; j < 3; j++) row[tets[4 * (b >> 2) + kFace[b & 3][j]]] = 0;
    uint32_t rows = 0;
    for (uint32_t v = 0; v < nv; v++)
        if (row[v] == 0) row[v] = static_cast<int32_t>(rows++);
    *nrows = rows;
    *ntri = static_cast<uint32_t>(boundary.size());
    if (!vis_verts) return 0;
    std::vector<uint8_t> done(rows, 0);
    for (uint32_t t = 0; t < nt; t++)   // ascending: the lowest tet containing the particle, its first corner there
        for (int k = 0; k < 4; k++) {
            const int32_t r = row[tets[4 * t + k]];
            if (r < 0 || done[r]) continue;
            done[r] = 1;
            vis_verts[4 * r] = static_cast<float>(t);
            for (int j = 0; j < 3; j++) vis_verts[4 * r + 1 + j] = j == k ? 1.0f : 0.0f;   // (corner 3: b3 = 1 - 0 - 0 - 0)
        }
    for (size_t i = 0; i < boundary.size(); i++) {
        const uint32_t t = static_cast<uint32_t>(boundary[i] >> 2), k = static_cast<uint32_t>(boundary[i] & 3);
        bool flip = false;
        if (verts) {
            const int32_t* c = tets + 4 * t;
            double m[3][3];
            for (int a = 0; a < 3; a++)
                for (int x = 0; x < 3; x++) m[a][x] = static_cast<double>(verts[3 * c[a + 1] + x]) - static_cast<double>(verts[3 * c[0] + x]);
            const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                               m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
            flip = det < 0.0;
        }
        const int32_t a = row[tets[4 * t + kFace[k][0]]], b = row[tets[4 * t + kFace[k][1]]], c2 = row[tets[4 * t + kFace[k][2]]];
        tri_ids[3 * i] = a;
        tri_ids[3 * i + 1] = flip ? c2 : b;
        tri_ids[3 * i + 2] = flip ? b : c2;
    }
    return 0;
}
int tetsim_prep_rest(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, double density, float* inv_mass, float* inv_rest_pose, float* inv_rest_volume) {
    if (!inv_mass || (nt && (!inv_rest_pose || !inv_rest_volume))) return TETSIM_EINVAL;
    std::string e = validate_mesh(verts, nv, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    prep_rest(verts, nv, tets, nt, density, inv_mass, inv_rest_pose, inv_rest_volume);
    return 0;
}

// the strain calls' per-tet records (strain.hip; include/tetsim.h: tetsim_prep_strain_table)
int tetsim_prep_strain_table(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, double density, void* records_out) {
    if (nt && !records_out) return TETSIM_EINVAL;
    std::string e = validate_mesh(verts, nv, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    std::vector<StrainRec> recs(nt);
    build_strain_table(verts, nv, tets, nt, density, recs.data());
    if (nt) std::memcpy(records_out, recs.data(), recs.size() * sizeof(StrainRec));
    return 0;
}

// the pose calls' per-particle records (pose.hip; include/tetsim.h: tetsim_prep_pose_table)
int tetsim_prep_pose_table(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, const uint32_t* body_first_vert, const uint32_t* body_first_tet,
                           uint32_t num_bodies, double density, void* records_out, double* centres_out) {
    if (nv && !records_out) return TETSIM_EINVAL;
    if ((body_first_vert == nullptr) != (body_first_tet == nullptr)) return fail(nullptr, TETSIM_EINVAL, "body_first_vert and body_first_tet must both be given or both be NULL");
    std::string e = validate_mesh(verts, nv, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    std::vector<uint32_t> fv = {0u, nv};
    if (body_first_vert) {
        if (!num_bodies) return fail(nullptr, TETSIM_EINVAL, "num_bodies is 0");
        if (body_first_tet[0] != 0 || body_first_vert[0] != 0 || body_first_tet[num_bodies] != nt || body_first_vert[num_bodies] != nv)
            return fail(nullptr, TETSIM_EINVAL, "body ranges must cover the whole mesh");
        for (uint32_t b = 0; b < num_bodies; b++) {
            if (body_first_tet[b] > body_first_tet[b + 1] || body_first_vert[b] > body_first_vert[b + 1]) return fail(nullptr, TETSIM_EINVAL, "body ranges must ascend");
            for (uint64_t i = 4ull * body_first_tet[b]; i < 4ull * body_first_tet[b + 1]; i++)
                if (static_cast<uint32_t>(tets[i]) < body_first_vert[b] || static_cast<uint32_t>(tets[i]) >= body_first_vert[b + 1])
                    return fail(nullptr, TETSIM_EINVAL, "a tet references a particle of another body");
        }
        fv.assign(body_first_vert, body_first_vert + num_bodies + 1);
    }
    std::vector<PoseRec> recs(nv);
    build_pose_table(verts, nv, tets, nt, fv.data(), static_cast<uint32_t>(fv.size() - 1), density, recs.data(), centres_out);
    if (nv) std::memcpy(records_out, recs.data(), recs.size() * sizeof(PoseRec));
    return 0;
}

// ---- the built-in partitioner (partitioner.cpp) -------------------------------------------------------------------
int tetsim_prep_partition(const float* verts, uint32_t nv, const int32_t* tets, uint32_t nt, int32_t part_count, int32_t* vert_owner_out) {
    if ((nt && !tets) || (nv && !vert_owner_out) || part_count < 1) return fail(nullptr, TETSIM_EINVAL, "tetsim_prep_partition: null argument or part_count < 1");
    if (verts)
        for (uint64_t i = 0; i < 3ull * nv; i++)
            if (!std::isfinite(verts[i])) return fail(nullptr, TETSIM_EINVAL, "non-finite vertex coordinate");
    const std::string e = prep_partition(verts, nv, tets, nt, part_count, vert_owner_out);
    return e.empty() ? TETSIM_OK : fail(nullptr, TETSIM_EINVAL, e);
}
int tetsim_prep_partition_quality(const int32_t* tets, uint32_t nt, uint32_t nv, int32_t part_count, const int32_t* vert_owner, TetSimPartQuality* out) {
    if ((nt && !tets) || !out || part_count < 1) return fail(nullptr, TETSIM_EINVAL, "tetsim_prep_partition_quality: null argument or part_count < 1");
    std::vector<int32_t> own;
    if (!vert_owner) {   // what tetsim_create / tetsim_plan_create pick by themselves
        own.resize(nv);
        const std::string e = prep_partition(nullptr, nv, tets, nt, part_count, own.data());
        if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
        vert_owner = own.data();
    }
    std::vector<PartQuality> q(part_count);
    const std::string e = partition_quality(tets, nt, nv, part_count, vert_owner, q.data());
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    for (int32_t r = 0; r < part_count; r++) {
        out[r].owned_particles = q[r].owned_particles; out[r].ghost_particles = q[r].ghost_particles; out[r].boundary_particles = q[r].boundary_particles;
        out[r].local_elems = q[r].local_elems; out[r].owned_elems = q[r].owned_elems; out[r].num_neighbours = q[r].num_neighbours;
    }
    return TETSIM_OK;
}

// ---- partition plan (host only) ---------------------------------------------------------------------------------
struct tetsim_plan_s { Partition P; };

int tetsim_plan_create(const int32_t* tets, uint32_t nt, uint32_t nv, int32_t part_count, int32_t part_index,
                       const int32_t* vert_owner, tetsim_plan* out) {
    if (!out) return fail(nullptr, TETSIM_EINVAL, "null plan pointer");
    *out = nullptr;
    std::string e = validate_mesh(reinterpret_cast<const float*>(tets), nv, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    tetsim_plan_s* p = new tetsim_plan_s();
    e = build_partition(tets, nt, nv, part_count, part_index, vert_owner, &p->P);
    if (!e.empty()) { delete p; return fail(nullptr, TETSIM_EINVAL, e); }
    *out = p;
    return 0;
}
int tetsim_plan_create_deep(const int32_t* tets, uint32_t nt, uint32_t nv, int32_t part_count, int32_t part_index,
                            const int32_t* vert_owner, int32_t depth, tetsim_plan* out) {
    if (!out) return fail(nullptr, TETSIM_EINVAL, "null plan pointer");
    *out = nullptr;
    std::string e = validate_mesh(reinterpret_cast<const float*>(tets), nv, tets, nt, false);
    if (!e.empty()) return fail(nullptr, TETSIM_EINVAL, e);
    tetsim_plan_s* p = new tetsim_plan_s();
    e = build_partition(tets, nt, nv, part_count, part_index, vert_owner, &p->P, depth);
    if (!e.empty()) { delete p; return fail(nullptr, TETSIM_EINVAL, e); }
    *out = p;
    return 0;
}
int tetsim_plan_layers(tetsim_plan p, uint32_t* first_layer_ghosts, uint8_t* tet_layer) {
    if (!p) return TETSIM_EINVAL;
    if (first_layer_ghosts) *first_layer_ghosts = p->P.n_ghost1;
    if (tet_layer) std::copy(p->P.tet_layer.begin(), p->P.tet_layer.end(), tet_layer);
    return 0;
}
int tetsim_plan_neighbour_layer2(tetsim_plan p, uint32_t i, uint32_t* send_count, uint32_t* recv_start, uint32_t* recv_count) {
    if (!p || i >= p->P.neigh.size()) return TETSIM_EINVAL;
    const auto& nb = p->P.neigh[i];
    if (send_count) *send_count = static_cast<uint32_t>(nb.send2_local.size());
    if (recv_start) *recv_start = nb.recv2_start;
    if (recv_count) *recv_count = nb.recv2_count;
    return 0;
}
int tetsim_plan_neighbour_layer2_ids(tetsim_plan p, uint32_t i, int32_t* send_local, int32_t* send_global, int32_t* recv_global) {
    if (!p || i >= p->P.neigh.size()) return TETSIM_EINVAL;
    const auto& nb = p->P.neigh[i];
    if (send_local) std::copy(nb.send2_local.begin(), nb.send2_local.end(), send_local);
    if (send_global) std::copy(nb.send2_global.begin(), nb.send2_global.end(), send_global);
    if (recv_global) std::copy(nb.recv2_global.begin(), nb.recv2_global.end(), recv_global);
    return 0;
}
void tetsim_plan_destroy(tetsim_plan p) { delete p; }
int tetsim_plan_sizes(tetsim_plan p, TetSimPlanSizes* out) {
    if (!p || !out) return TETSIM_EINVAL;
    out->owned_particles = p->P.n_owned;
    out->boundary_particles = p->P.n_boundary;
    out->local_particles = static_cast<uint32_t>(p->P.local_to_global_vert.size());
    out->local_elems = static_cast<uint32_t>(p->P.local_to_global_tet.size());
    out->owned_elems = p->P.owned_tets;
    out->num_neighbours = static_cast<uint32_t>(p->P.neigh.size());
    return 0;
}
int tetsim_plan_arrays(tetsim_plan p, int32_t* l2gv, int32_t* l2gt, int32_t* ltets) {
    if (!p) return TETSIM_EINVAL;
    if (l2gv) std::copy(p->P.local_to_global_vert.begin(), p->P.local_to_global_vert.end(), l2gv);
    if (l2gt) std::copy(p->P.local_to_global_tet.begin(), p->P.local_to_global_tet.end(), l2gt);
    if (ltets) std::copy(p->P.local_tets.begin(), p->P.local_tets.end(), ltets);
    return 0;
}
int tetsim_plan_neighbour(tetsim_plan p, uint32_t i, int32_t* rank, uint32_t* send_count, uint32_t* recv_start,
                          uint32_t* recv_count, int32_t* contiguous) {
    if (!p || i >= p->P.neigh.size()) return TETSIM_EINVAL;
    const auto& nb = p->P.neigh[i];
    if (rank) *rank = nb.rank;
    if (send_count) *send_count = static_cast<uint32_t>(nb.send_local.size());
    if (recv_start) *recv_start = nb.recv_start;
    if (recv_count) *recv_count = nb.recv_count;
    if (contiguous) *contiguous = nb.send_contiguous ? 1 : 0;
    return 0;
}
int tetsim_plan_neighbour_ids(tetsim_plan p, uint32_t i, int32_t* send_local, int32_t* send_global, int32_t* recv_global) {
    if (!p || i >= p->P.neigh.size()) return TETSIM_EINVAL;
    const auto& nb = p->P.neigh[i];
    if (send_local) std::copy(nb.send_local.begin(), nb.send_local.end(), send_local);
    if (send_global) std::copy(nb.send_global.begin(), nb.send_global.end(), send_global);
    if (recv_global) std::copy(nb.recv_global.begin(), nb.recv_global.end(), recv_global);
    return 0;
}

}  // extern "C"
