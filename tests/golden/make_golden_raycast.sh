#!/usr/bin/env bash
# Records the ray-cast fixtures (run in the BUILD container only: needs the reference's node_modules and node).
# Copies three.js into a scratch directory (never into the repo), marks it an ES module and runs make_golden_raycast.mjs,
# which casts rays against the committed dragon_vispos_10.f32 / dragon_vistris.u16 and writes DATA fixtures next to itself.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
REF=${REF:-/root/reference}
SCRATCH=$(mktemp -d /tmp/tetsim_ref.XXXXXX)
trap 'rm -rf "$SCRATCH"' EXIT
mkdir -p "$SCRATCH/node_modules/three/build"
cp "$REF/node_modules/three/build/three.module.js" "$SCRATCH/node_modules/three/build/"
echo '{"type":"module"}' > "$SCRATCH/package.json"
echo '{"type":"module"}' > "$SCRATCH/node_modules/three/package.json"
cp "$HERE/make_golden_raycast.mjs" "$SCRATCH/"
node "$SCRATCH/make_golden_raycast.mjs" "$SCRATCH" "$HERE"
