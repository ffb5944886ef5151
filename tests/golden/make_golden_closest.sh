#!/usr/bin/env bash
# Records the closest-point fixture (run in the BUILD container only: needs the reference's node_modules and node).
# Copies three.js into a scratch directory (never into the repo), marks it an ES module and runs make_golden_closest.mjs,
# which asks Triangle.closestPointToPoint about seeded (triangle, point) pairs and writes closest_three.json (DATA) next to itself.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REF=${REF:?set REF to the reference checkout (its node_modules hold three.js r160)}
SCRATCH=$(mktemp -d /tmp/tetsim_ref.XXXXXX)
trap 'rm -rf "$SCRATCH"' EXIT
mkdir -p "$SCRATCH/node_modules/three/build"
cp "$REF/node_modules/three/build/three.module.js" "$SCRATCH/node_modules/three/build/"
echo '{"type":"module"}' > "$SCRATCH/package.json"
echo '{"type":"module"}' > "$SCRATCH/node_modules/three/package.json"
cp "$HERE/make_golden_closest.mjs" "$SCRATCH/"
node "$SCRATCH/make_golden_closest.mjs" "$SCRATCH" "$HERE"
