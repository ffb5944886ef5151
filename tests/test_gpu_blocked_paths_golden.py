"""The blocked polar kernels (pj_blocked.hip) bit for bit against tests/golden/blocked_paths_bits.json, recorded by
tools/record_blocked_paths.py from the build whose source_sha the file names: positions, velocities and quaternions after 25 substeps with a
collider and a grab, for the three tet records on the four unpartitioned paths -- the tetsim_step pair, the fused kernel, the persistent
frame kernel (one-XCD placement where the device has it: lat5, hub, wheel; any-XCD placement: lat16) and the one-launch call.  The other
tests of these kernels compare one path with another, which a change made to a step they share passes; here the bits themselves are held.
The paths are chosen by switches the library reads once per process, so the recording runs in two child processes (the tool's, imported
here: the file and the test cannot drift apart), once for all cases.  The file is never recorded again: a difference is a change of the
arithmetic, of an order of additions or of what a kernel stages.  The halo variants are held by the partition tests (test_gpu_polar.py,
test_gpu_p2p_halo.py), which compare against the monolithic body pinned here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_blocked_paths", os.path.join(ROOT, "tools", "record_blocked_paths.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        doc = json.load(f)
    assert sorted(doc["cases"]) == sorted(rec.MESHES) and doc["seeds"] == rec.SEEDS and doc["modes"] == list(rec.MODES)
    assert doc["paths"] == rec.PATHS and doc["calls"] == list(rec.CALLS)
    return doc["cases"]


@pytest.fixture(scope="module")
def recorded():
    return rec.record_all()


@pytest.mark.parametrize("path", rec.PATHS)
@pytest.mark.parametrize("mode", list(rec.MODES))
@pytest.mark.parametrize("name", rec.MESHES)
def test_paths_equal_the_recorded_bits(golden, recorded, name, mode, path):
    got, want = recorded[path][name][mode], golden[name][mode]
    assert got["info"] == rec.PATH_CODE[path], (name, mode, path, got["info"])
    for what in ("pos", "vel", "quats"):
        if isinstance(want[what], dict):
            assert got[what] == want[what], (name, mode, path, what)
            continue
        bad = [i for i, (g, w) in enumerate(zip(got[what], want[what])) if g != w]
        assert len(got[what]) == len(want[what]) and bad == [], (name, mode, path, what, len(bad), [(i, got[what][i], want[what][i]) for i in bad[:2]])
