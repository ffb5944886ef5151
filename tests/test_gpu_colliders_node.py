"""Kinematic colliders through the Node.js boundary: SoftBodyHIP.js setColliders ({x, y, z} objects, N-API) and the Python host's
setColliders give the same trajectory bit for bit (tetsim_amd/node/test_colliders.js)."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, load_mesh
from tetsim_amd import SoftBodyHIP

NODE = shutil.which("node")
NODE_DIR = os.path.join(ROOT, "tetsim_amd", "node")
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1.0 / 100000.0, volCompliance=0.0,
          worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])
DT = (1.0 / 60.0) / 20


def scene(frame):   # test_colliders.js's scene, number for number
    t = frame * 20 * DT
    return [
        dict(kind="sphere", a=[-0.3 + 0.2 * t, 0.17, -0.1 * t], radius=0.12, friction=200.0, velocity=[0.2, 0.0, -0.1]),
        dict(kind="capsule", a=[0.1, 0.24, -0.3], b=[0.5, 0.21, 0.3], radius=0.04, friction=50.0),
        dict(kind="box", a=[0.0, 0.1, 0.1], b=[0.6, 0.05, 0.15], axes=[[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]], friction=1000.0),
        dict(kind="plane", a=[0.0, 0.08, 0.0], b=[0.2, 1.0, 0.1], friction=5.0),
    ]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed on this host")
def test_node_set_colliders_matches_the_python_host_bit_for_bit():
    from tetsim_amd.node.build_addon import build_addon
    build_addon()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pos.f32")
        r = subprocess.run([NODE, os.path.join(NODE_DIR, "test_colliders.js"), out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "node colliders ok" in r.stdout, r.stdout + r.stderr
        js = np.fromfile(out, dtype="<f4").reshape(-1, 3)
    v, t = load_mesh("dragon")
    v = v.copy()
    v[:, 1] = v[:, 1] + np.float32(0.3 - float(v[:, 1].min()))
    body = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    for f in range(8):
        body.setColliders(scene(f))
        body.simulateSubsteps(20, DT, PP)
    py = body.pos
    assert np.array_equal(js.view(np.uint32), py.view(np.uint32))
    assert py[:, 1].min() < 0.25   # it reached the colliders
