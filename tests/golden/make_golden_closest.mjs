// Records what three.js r160's Triangle.closestPointToPoint answers for (triangle, point) pairs (tests/golden/make_golden_closest.sh).
//   node make_golden_closest.mjs <scratch with node_modules/three> <tests/golden>
// Output: closest_three.json -- {three, counts, regions, cases: [{kind, t: [9], p: [3], q: [3], region}]}; every number a double as 16 hex
//         digits of its bits (t: the corners a, b, c, each an f32 value; p: the point; q: three.js's answer).
// `region` is not three.js's (the method returns the point alone): it is the branch the method's own comparisons take, evaluated here with
// the same Vector3 operations -- 1, 2, 3 the vertices a, b, c; 4, 5, 6 the edges ab, ac, bc; 0 the face.
import { writeFileSync } from 'fs';
import { join, resolve } from 'path';
import { pathToFileURL } from 'url';

const [scratch, out] = process.argv.slice(2).map((p) => resolve(p));
import(pathToFileURL(join(scratch, 'node_modules/three/build/three.module.js')).href).then((THREE) => {

let seed = 20250917;   // mulberry32
const rnd = () => { seed = (seed + 0x6D2B79F5) | 0; let t = Math.imul(seed ^ (seed >>> 15), 1 | seed); t = (t + Math.imul(t ^ (t >>> 7), 61 | t)) ^ t; return ((t ^ (t >>> 14)) >>> 0) / 4294967296; };
const V = (x, y, z) => new THREE.Vector3(x, y, z);
const f32 = (v) => V(Math.fround(v.x), Math.fround(v.y), Math.fround(v.z));
const sym = () => 2 * rnd() - 1;
const hex = (x) => { const b = Buffer.alloc(8); b.writeDoubleBE(x); return b.toString('hex'); };

function regionOf(a, b, c, p) {   // the comparisons of Triangle.closestPointToPoint, in its order
    const ab = V().subVectors(b, a), ac = V().subVectors(c, a), ap = V().subVectors(p, a);
    const d1 = ab.dot(ap), d2 = ac.dot(ap);
    if (d1 <= 0 && d2 <= 0) return 1;
    const bp = V().subVectors(p, b);
    const d3 = ab.dot(bp), d4 = ac.dot(bp);
    if (d3 >= 0 && d4 <= d3) return 2;
    const vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) return 4;
    const cp = V().subVectors(p, c);
    const d5 = ab.dot(cp), d6 = ac.dot(cp);
    if (d6 >= 0 && d5 <= d6) return 3;
    const vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) return 5;
    const va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) return 6;
    return 0;
}

const cases = [];
function add(kind, a, b, c, p) {
    const q = new THREE.Triangle(a, b, c).closestPointToPoint(p, V());
    cases.push({ kind, t: [a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z].map(hex), p: [p.x, p.y, p.z].map(hex), q: [q.x, q.y, q.z].map(hex), region: regionOf(a, b, c, p) });
}
const triangle = (scale, shift) => [0, 1, 2].map(() => f32(V(sym() * scale + shift, sym() * scale + shift, sym() * scale + shift)));
const at = (a, b, c, u, v, w, h) => {   // u a + v b + w c + h n, n the unit normal
    const n = V().crossVectors(V().subVectors(b, a), V().subVectors(c, a));
    if (n.length() > 0) n.normalize();
    return V().addScaledVector(a, u).addScaledVector(b, v).addScaledVector(c, w).addScaledVector(n, h);
};
// barycentric coordinates that aim at each region (the recorded region is the one the method takes, whatever was aimed at)
const aim = [
    () => { const v = rnd(), w = rnd() * (1 - v); return [1 - v - w, v, w]; },                        // 0 face
    () => { const v = -rnd(), w = -rnd(); return [1 - v - w, v, w]; },                                // 1 vertex a
    () => { const u = -rnd(), w = -rnd(); return [u, 1 - u - w, w]; },                                // 2 vertex b
    () => { const u = -rnd(), v = -rnd(); return [u, v, 1 - u - v]; },                                // 3 vertex c
    () => { const v = 0.1 + 0.8 * rnd(), w = -0.3 * rnd(); return [1 - v - w, v, w]; },               // 4 edge ab
    () => { const w = 0.1 + 0.8 * rnd(), v = -0.3 * rnd(); return [1 - v - w, v, w]; },               // 5 edge ac
    () => { const w = 0.1 + 0.8 * rnd(), u = -0.3 * rnd(); return [u, 1 - u - w, w]; },               // 6 edge bc
];
for (let r = 0; r < 7; r++)
    for (let i = 0; i < 36; i++) {
        const [a, b, c] = triangle(1, 0), [u, v, w] = aim[r]();
        add('random', a, b, c, at(a, b, c, u, v, w, sym()));
    }
for (let i = 0; i < 30; i++) {       // exactly on a vertex
    const [a, b, c] = triangle(1, 0);
    add('on_vertex', a, b, c, [a, b, c][i % 3].clone());
}
for (let i = 0; i < 30; i++) {       // on an edge: the midpoint (exact or rounded once), and a point a + t (b - a)
    const [a, b, c] = triangle(1, 0), e = [[a, b], [a, c], [b, c]][i % 3];
    add('on_edge', a, b, c, i % 2 ? V().addVectors(e[0], e[1]).multiplyScalar(0.5) : V().subVectors(e[1], e[0]).multiplyScalar(rnd()).add(e[0]));
}
for (let i = 0; i < 30; i++) {       // in the plane: inside, and outside beside an edge or a vertex
    const [a, b, c] = triangle(1, 0), [u, v, w] = aim[i % 7]();
    add('in_plane', a, b, c, at(a, b, c, u, v, w, 0));
}
for (let i = 0; i < 42; i++) {       // zero area: two or three corners equal, or three on a line
    let [a, b, c] = triangle(1, 0);
    const m = i % 6;
    if (m === 0) b = a.clone();
    else if (m === 1) c = a.clone();
    else if (m === 2) c = b.clone();
    else if (m === 3) { b = a.clone(); c = a.clone(); }
    else if (m === 4) c = f32(V(2 * b.x - a.x, 2 * b.y - a.y, 2 * b.z - a.z));     // c beyond b (collinear up to the f32 rounding)
    else { a = f32(V(0.25 * (i + 1), 0.5, -0.125)); b = V(a.x + 0.5, a.y, a.z); c = V(a.x + 0.25, a.y, a.z); }   // exactly collinear, c between
    add('degenerate', a, b, c, i % 7 === 0 ? a.clone() : V(sym(), sym(), sym()));
}
for (let i = 0; i < 42; i++) {       // coordinates near 1e3: small triangles far from the origin, points near and far
    const [a, b, c] = triangle(i % 2 ? 0.01 : 1, 1000), [u, v, w] = aim[i % 7]();
    add('near_1e3', a, b, c, at(a, b, c, u, v, w, i % 3 ? sym() * 0.01 : sym() * 1000));
}

const regions = [0, 0, 0, 0, 0, 0, 0], counts = {};
for (const k of cases) { regions[k.region]++; counts[k.kind] = (counts[k.kind] || 0) + 1; }
if (regions.some((n) => n < 20)) throw new Error('a region appears fewer than 20 times: ' + regions);
writeFileSync(join(out, 'closest_three.json'), JSON.stringify({ three: THREE.REVISION, counts, regions, cases }, null, 0).replace(/\},\{/g, '},\n{') + '\n');
console.log(`three r${THREE.REVISION}: ${cases.length} pairs, regions`, regions, counts);
});
