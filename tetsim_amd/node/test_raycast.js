'use strict';
// Picking through the N-API boundary (run on a GPU host):  node tetsim_amd/node/test_raycast.js
// The Dragon (Neo-Hookean PRECISE) after 10 substeps has the visual positions of tests/golden/dragon_vispos_10.f32; the addon's
// raycastVisual and SoftBodyHIP.raycast must return the winners three.js r160 recorded for the rays of raycast_dragon_rays.f64
// (tests/golden/make_golden_raycast.sh), bit for bit, and the bounding sphere must be three's.
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const { SoftBodyHIP } = require('./SoftBodyHIP.js');

const G = path.join(__dirname, '..', '..', 'tests', 'golden');
const raw = n => { const b = fs.readFileSync(path.join(G, n)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); };
const verts = new Float32Array(raw('dragon_verts.f32')), tets = Array.from(new Int32Array(raw('dragon_tets.i32')));
const vis = new Float32Array(raw('dragon_vis.f32')), tris = Array.from(new Uint16Array(raw('dragon_vistris.u16')));
const rays = new Float64Array(raw('raycast_dragon_rays.f64')), h64 = new Float64Array(raw('raycast_dragon_hits.f64'));
const h32 = new Int32Array(raw('raycast_dragon_hits.i32')), sphere = new Float64Array(raw('raycast_dragon_sphere.f64'));
const same = (a, b) => Buffer.compare(Buffer.from(Float64Array.of(a).buffer), Buffer.from(Float64Array.of(b).buffer)) === 0;   // as bits

const pp = { gravity: -9.81, friction: 1000.0, density: 1000.0, devCompliance: 1e-5, volCompliance: 0.0,
             worldBounds: [-2.5, -1.0, -2.5, 2.5, 10.0, 2.5], tetsim: { solver: 'neohookean', precision: 'precise' } };
const body = new SoftBodyHIP(verts, tets, [], pp, vis, tris, null);
const dt = (1.0 * (1.0 / 60.0)) / 10;
for (let s = 0; s < 10; s++) body.simulate(dt, pp);

// the addon: the 480 rays that share near = 0, far = Infinity in one call
const n = 480, o = new Float64Array(3 * n), d = new Float64Array(3 * n);
for (let i = 0; i < n; i++) {
    assert(rays[8 * i + 6] === 0 && rays[8 * i + 7] === Infinity);
    for (let k = 0; k < 3; k++) { o[3 * i + k] = rays[8 * i + k]; d[3 * i + k] = rays[8 * i + 3 + k]; }
}
const res = body._api.raycastVisual(body._h, o, d, 0, Infinity);
let hits = 0;
for (let i = 0; i < n; i++) {
    assert.strictEqual(res.ints[4 * i], h32[2 * i], 'hit of ray ' + i);
    assert.strictEqual(res.ints[4 * i + 2], h32[2 * i + 1], 'faceIndex of ray ' + i);
    for (let k = 0; k < 4; k++) assert(same(res.reals[4 * i + k], h64[4 * i + k]), 'distance / point of ray ' + i);
    hits += res.ints[4 * i];
}
assert(hits >= 120);
// SoftBodyHIP.raycast(raycaster): every recorded ray, the windowed ones included, as a Raycaster-shaped object
for (let i = 0; i < rays.length / 8; i++) {
    const r = rays.subarray(8 * i, 8 * i + 8);
    const hit = body.raycast({ ray: { origin: { x: r[0], y: r[1], z: r[2] }, direction: { x: r[3], y: r[4], z: r[5] } }, near: r[6], far: r[7] });
    if (!h32[2 * i]) { assert.strictEqual(hit, null, 'ray ' + i + ' misses'); continue; }
    assert(hit !== null && hit.faceIndex === h32[2 * i + 1] && same(hit.distance, h64[4 * i]), 'winner of ray ' + i);
    assert(same(hit.point.x, h64[4 * i + 1]) && same(hit.point.y, h64[4 * i + 2]) && same(hit.point.z, h64[4 * i + 3]), 'point of ray ' + i);
}
const s = body._api.readVisualBoundingSphere(body._h);
for (let k = 0; k < 4; k++) assert(same(s[k], sphere[k]), 'bounding sphere');
// startGrabRay: the particle startGrab finds for the f32 hit point
const r = rays.subarray(8 * 384, 8 * 384 + 8);
const caster = { ray: { origin: { x: r[0], y: r[1], z: r[2] }, direction: { x: r[3], y: r[4], z: r[5] } }, near: 0, far: Infinity };
const first = body.raycast(caster), grabbed = body.startGrabRay(caster);
assert(first !== null && grabbed !== null && grabbed.faceIndex === first.faceIndex && same(grabbed.distance, first.distance));
const id = body.grabId;
body.startGrab({ x: r[0] + r[3] * first.distance, y: r[1] + r[4] * first.distance, z: r[2] + r[5] * first.distance });
assert(id >= 0 && body.grabId === id);
assert.strictEqual(body.startGrabRay({ ray: { origin: { x: 0, y: 50, z: 0 }, direction: { x: 0, y: 1, z: 0 } }, near: 0, far: Infinity }), null);
assert.strictEqual(body.grabId, id);   // a miss leaves the grab as it was
assert.throws(() => body.raycast({ ray: { origin: { x: 0, y: 0, z: 0 }, direction: { x: 0, y: 0, z: 0 } }, near: 0, far: 1 }), /zero direction/);
// endFrame() with an injected three.js that has a Sphere class: visMesh.geometry.boundingSphere comes from the device (three's bits)
{
    class Vector3 { constructor(x = 0, y = 0, z = 0) { this.x = x; this.y = y; this.z = z; } set(x, y, z) { this.x = x; this.y = y; this.z = z; return this; } }
    class Sphere { constructor() { this.center = new Vector3(); this.radius = -1; } }
    class BufferAttribute { constructor(array, itemSize) { this.array = array; this.itemSize = itemSize; this.needsUpdate = false; } }
    let own = 0;
    class BufferGeometry {
        constructor() { this.attributes = {}; this.index = null; this.boundingSphere = null; }
        setAttribute(name, a) { this.attributes[name] = a; return this; }
        setIndex(ids) { this.index = ids; return this; }
        computeVertexNormals() { if (!this.attributes.normal) this.attributes.normal = new BufferAttribute(new Float32Array(this.attributes.position.array.length), 3); }
        computeBoundingSphere() { if (this.attributes.position.array.length === 3 * 29800) own++; }
    }
    class Layers { constructor() { this.mask = 1; } enable(l) { this.mask |= 1 << l; } }
    class Object3D { constructor(geometry, material) { this.geometry = geometry; this.material = material; this.layers = new Layers(); this.userData = {}; this.visible = true; } }
    const THREE = { BufferAttribute, BufferGeometry, LineSegments: Object3D, Mesh: Object3D, Sphere, Vector3 };
    const shown = new SoftBodyHIP(verts.slice(0), tets, [0, 1, 1, 2], pp, vis, tris, {}, { THREE });
    for (let s = 0; s < 10; s++) shown.simulate(dt, pp);
    shown.endFrame();
    const bs = shown.visMesh.geometry.boundingSphere;
    assert(bs instanceof Sphere && same(bs.center.x, sphere[0]) && same(bs.center.y, sphere[1]) && same(bs.center.z, sphere[2]) && same(bs.radius, sphere[3]), 'endFrame bounding sphere');
    assert.strictEqual(own, 0, 'the visual mesh\'s computeBoundingSphere must come from the device');
    const hit = shown.raycast({ ray: { origin: { x: r[0], y: r[1], z: r[2] }, direction: { x: r[3], y: r[4], z: r[5] } }, near: 0, far: Infinity });
    assert(hit.point instanceof Vector3 && hit.object === shown.visMesh && hit.faceIndex === first.faceIndex);
    shown.dispose();
}
body.dispose();
console.log('node raycast ok');
