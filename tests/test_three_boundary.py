"""The JavaScript boundary against the REAL three.js (missing #3): `.edgeMesh` / `.visMesh` of SoftBodyHIP built with
the three r160 module the reference itself vendors (node_modules/three), not with a stand-in -- LineSegments / Mesh
instances, layer 1 against a layer-1 Raycaster, userData, the position attribute aliasing the caller's array, version counters behind
`needsUpdate`, and a Raycaster.intersectObjects -> startGrab round trip as Grabber.start does (Softbody.js:36-57, 440-456; main.js:60-68).
CPU only: the native addon is replaced by a 2-tet stand-in inside the node script.  The module is the working copy build() stages under
oracle/_ref/ (oracle/glsl_ref/build.sh, where the reference is present); three.js is imported from a scratch copy of it, nothing of it
is committed or shipped."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

THREE_MODULE = os.path.join(ROOT, "oracle", "_ref", "three.module.js")
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None or not os.path.exists(THREE_MODULE), reason="needs node and the reference's vendored three.js, staged by build() under oracle/_ref/")
def test_display_objects_against_the_reference_s_own_three_js(tmp_path):
    build = tmp_path / "node_modules" / "three" / "build"
    build.mkdir(parents=True)
    shutil.copy(THREE_MODULE, build / "three.module.js")
    (tmp_path / "node_modules" / "three" / "package.json").write_text('{"type":"module"}')
    r = subprocess.run([NODE, os.path.join(ROOT, "tetsim_amd", "node", "test_three_boundary.mjs"), str(build / "three.module.js")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "THREE_BOUNDARY_OK r160" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
