// Records what three.js r160 answers for ray casts against the Dragon's visual mesh (tests/golden/make_golden_raycast.sh).
//   node make_golden_raycast.mjs <scratch with node_modules/three> <tests/golden>
// Input : dragon_vispos_10.f32 (29,800 visual vertices after 10 substeps), dragon_vistris.u16 (59,657 triangles).
// Output: raycast_dragon_rays.f64  [512][8]  origin, direction, near, far
//         raycast_dragon_hits.f64  [512][4]  distance, point            (zeros on a miss)
//         raycast_dragon_hits.i32  [512][2]  hit, faceIndex             (faceIndex -1 on a miss)
//         raycast_dragon_sphere.f64 [4]      BufferGeometry.computeBoundingSphere(): centre, radius
//         golden_raycast.json                hashes and counts
// Every ray goes through `new Raycaster(origin, direction, near, far).intersectObject(mesh)` on a Mesh with an identity world
// matrix and a front-side material; the FIRST entry of the (stably sorted) result is recorded.
import { createHash } from 'crypto';
import { readFileSync, writeFileSync } from 'fs';
import { join, resolve } from 'path';
import { pathToFileURL } from 'url';

const [scratch, out] = process.argv.slice(2).map((p) => resolve(p));
import(pathToFileURL(join(scratch, 'node_modules/three/build/three.module.js')).href).then((THREE) => {

const f32 = (name) => { const b = readFileSync(join(out, name)); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };
const pos = f32('dragon_vispos_10.f32');
const tb = readFileSync(join(out, 'dragon_vistris.u16'));
const tris = new Uint16Array(tb.buffer.slice(tb.byteOffset, tb.byteOffset + tb.length));
const nv = pos.length / 3;

const geometry = new THREE.BufferGeometry();
geometry.setAttribute('position', new THREE.BufferAttribute(pos, 3));
geometry.setIndex(new THREE.BufferAttribute(tris, 1));
const mesh = new THREE.Mesh(geometry, new THREE.MeshBasicMaterial({ side: THREE.FrontSide }));
mesh.updateMatrixWorld(true);
geometry.computeBoundingSphere();
const C = geometry.boundingSphere.center, R = geometry.boundingSphere.radius;

let seed = 20240611;   // mulberry32
const rnd = () => { seed = (seed + 0x6D2B79F5) | 0; let t = Math.imul(seed ^ (seed >>> 15), 1 | seed); t = (t + Math.imul(t ^ (t >>> 7), 61 | t)) ^ t; return ((t ^ (t >>> 14)) >>> 0) / 4294967296; };
const unit = () => { for (;;) { const v = new THREE.Vector3(2 * rnd() - 1, 2 * rnd() - 1, 2 * rnd() - 1); const l = v.length(); if (l > 1e-3 && l <= 1) return v.divideScalar(l); } };
const ball = () => { for (;;) { const v = new THREE.Vector3(2 * rnd() - 1, 2 * rnd() - 1, 2 * rnd() - 1); if (v.length() <= 1) return v; } };

const rays = [];
for (let i = 0; i < 384; i++) {      // from a sphere of three radii, aimed at a random point inside the bounding sphere
    const o = unit().multiplyScalar(3 * R).add(C), t = ball().multiplyScalar(R).add(C);
    rays.push({ o, d: t.sub(o).normalize(), near: 0, far: Infinity });
}
for (let i = 0; i < 96; i++) {       // straight at a vertex: the triangles around it meet the ray at one point
    const v = Math.floor(rnd() * nv);
    rays.push({ o: new THREE.Vector3(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2] + 5), d: new THREE.Vector3(0, 0, -1), near: 0, far: Infinity });
}
const cast = (r) => new THREE.Raycaster(r.o, r.d, r.near, r.far).intersectObject(mesh);
// finite windows: cut the first front face away (a later one wins, or none), cut everything, or put the window's edge on the winner
const bases = rays.map((r) => [r, [...new Set(cast(r).map((h) => h.distance))]]).filter(([, d]) => d.length > 0);
const deep = bases.filter(([, d]) => d.length > 1), flat = bases.filter(([, d]) => d.length === 1);
for (let j = 0; j < 32; j++) {
    const mode = j % 4;
    const pool = (mode === 0 || mode === 2) && j < 24 ? deep : (j % 8 < 4 ? deep : flat);
    const [r, d] = pool[Math.floor(rnd() * pool.length)];
    const mid = d.length > 1 ? 0.5 * (d[0] + d[1]) : d[0] + 0.01;
    let near = 0, far = Infinity;
    if (mode === 0) near = mid;
    else if (mode === 1) far = 0.5 * d[0];
    else if (mode === 2) { near = mid; far = d.length > 2 ? 0.5 * (d[1] + d[2]) : mid + 10; }
    else { near = d[0]; far = d[0]; }
    rays.push({ o: r.o.clone(), d: r.d.clone(), near, far });
}

const n = rays.length;
const R64 = new Float64Array(8 * n), H64 = new Float64Array(4 * n), H32 = new Int32Array(2 * n);
let hits = 0, ties = 0;
rays.forEach((r, i) => {
    R64.set([r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, r.near, r.far], 8 * i);
    const res = cast(r);
    H32[2 * i + 1] = -1;
    if (res.length) {
        hits++;
        if (res.length > 1 && res[1].distance === res[0].distance) ties++;
        H32[2 * i] = 1; H32[2 * i + 1] = res[0].faceIndex;
        H64.set([res[0].distance, res[0].point.x, res[0].point.y, res[0].point.z], 4 * i);
    }
});
const S64 = new Float64Array([C.x, C.y, C.z, R]);
const files = { 'raycast_dragon_rays.f64': R64, 'raycast_dragon_hits.f64': H64, 'raycast_dragon_hits.i32': H32, 'raycast_dragon_sphere.f64': S64 };
const sha = {};
for (const [name, a] of Object.entries(files)) {
    const b = Buffer.from(a.buffer, a.byteOffset, a.byteLength);
    writeFileSync(join(out, name), b);
    sha[name] = createHash('sha256').update(b).digest('hex');
}
writeFileSync(join(out, 'golden_raycast.json'), JSON.stringify({
    three: THREE.REVISION, rays: n, random: 384, at_vertex: 96, windowed: 32, hits, winners_tied: ties,
    sphere: { centre: [C.x, C.y, C.z], radius: R }, sha256: sha,
}, null, 1) + '\n');
console.log(`three r${THREE.REVISION}: ${n} rays, ${hits} hit, ${ties} winners tied; sphere`, C.x, C.y, C.z, R);
});
