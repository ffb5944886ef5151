"""Picking through the Node.js boundary: the addon's raycastVisual, SoftBodyHIP.raycast / startGrabRay and the device bounding
sphere return what three.js r160 recorded for the fixture rays (tetsim_amd/node/test_raycast.js)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
NODE_DIR = os.path.join(ROOT, "tetsim_amd", "node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node is not installed on this host")
def test_node_raycast_returns_the_threejs_winners():
    from tetsim_amd.node.build_addon import build_addon
    build_addon()
    r = subprocess.run([NODE, os.path.join(NODE_DIR, "test_raycast.js")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "node raycast ok" in r.stdout, r.stdout + r.stderr
