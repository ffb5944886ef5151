'use strict';
// Kinematic colliders through the N-API boundary (run on a GPU host):  node tetsim_amd/node/test_colliders.js OUT.f32
// A Dragon (polar FAST) lands on a sphere, a capsule, a rotated box and a tilted plane given as {x, y, z} objects, one moving with
// its velocity set; the positions after 8 frames of 20 substeps go to OUT.f32 (tests/test_gpu_colliders_node.py runs the same
// scene through the Python host and compares them bit for bit).
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const { SoftBodyHIP } = require('./SoftBodyHIP.js');

const G = path.join(__dirname, '..', '..', 'tests', 'golden');
const f32 = n => { const b = fs.readFileSync(path.join(G, n)); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const i32 = n => { const b = fs.readFileSync(path.join(G, n)); return new Int32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const verts = f32('dragon_verts.f32'), tets = Array.from(i32('dragon_tets.i32'));
let ymin = Infinity;
for (let i = 1; i < verts.length; i += 3) ymin = Math.min(ymin, verts[i]);
const lift = Math.fround(0.3 - ymin);   // (the Python side: v[:, 1] += float32(0.3) - min, in f32)
for (let i = 1; i < verts.length; i += 3) verts[i] = Math.fround(verts[i] + lift);
const pp = { gravity: -9.81, friction: 1000.0, density: 1000.0, devCompliance: 1.0 / 100000.0, volCompliance: 0.0,
             worldBounds: [-2.5, -1.0, -2.5, 2.5, 10.0, 2.5], tetsim: { solver: 'polar', precision: 'fast' } };
const dt = (1.0 / 60.0) / 20;
const scene = frame => {
    const t = frame * 20 * dt;
    return [
        { kind: 'sphere', a: { x: -0.3 + 0.2 * t, y: 0.17, z: -0.1 * t }, radius: 0.12, friction: 200.0, velocity: { x: 0.2, y: 0.0, z: -0.1 } },
        { kind: 'capsule', a: { x: 0.1, y: 0.24, z: -0.3 }, b: { x: 0.5, y: 0.21, z: 0.3 }, radius: 0.04, friction: 50.0 },
        { kind: 'box', a: { x: 0.0, y: 0.1, z: 0.1 }, b: { x: 0.6, y: 0.05, z: 0.15 }, axes: [{ x: 0.8, y: 0.0, z: -0.6 }, { x: 0.0, y: 1.0, z: 0.0 }, { x: 0.6, y: 0.0, z: 0.8 }], friction: 1000.0 },
        { kind: 'plane', a: { x: 0.0, y: 0.08, z: 0.0 }, b: { x: 0.2, y: 1.0, z: 0.1 }, friction: 5.0 },
    ];
};
const body = new SoftBodyHIP(verts, tets, [], pp, new Float32Array(0), [], null);
assert.throws(() => body.setColliders([{ kind: 'plane', b: { x: 0, y: 0, z: 0 } }]), /zero-length plane normal/);
for (let f = 0; f < 8; f++) {
    body.setColliders(scene(f));
    body.simulateSubsteps(20, dt, pp);
    body.endFrame();
}
fs.writeFileSync(process.argv[2], Buffer.from(body.pos.buffer, body.pos.byteOffset, body.pos.byteLength));
body.dispose();
console.log('node colliders ok');
