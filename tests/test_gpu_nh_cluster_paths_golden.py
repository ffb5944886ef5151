"""The four-lane Neo-Hookean cluster kernels (nh_kernels.inc) bit for bit against tests/golden/nh_cluster_paths_bits.json, recorded by
tools/record_nh_cluster_paths.py from the build whose source_sha the file names: positions, velocities, previous positions and volError
after 26 substeps with a collider and a grab, on the per-colour launches (nh_cluster4_kernel, FAST and PRECISE; on lat30 PRECISE is the
one-lane nh_cluster_kernel), the one-launch sweep (nh_sweep1_kernel, with and without the folded particle pass) and the one-launch call
(nh_call_kernel).  The other tests of these kernels compare one path with its twin, which a change made to a step they share passes; here
the bits themselves are held.  The recording is the tool's, imported here: the file and the test cannot drift apart.  It follows every call
with sync(), which raises where a cluster waited in vain -- the body would go on with one launch per colour, whose bits are the same, and
the test would pass on the fall-back (TetSimInfo has no field for the one-launch sweep; tetsim_sync's error is how a body reports that it
left it).  The file is never recorded again: a difference is a change of the arithmetic or of the order of the solves."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_nh_cluster_paths", os.path.join(ROOT, "tools", "record_nh_cluster_paths.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        doc = json.load(f)
    assert sorted(doc["cases"]) == sorted(rec.MESHES) and doc["seeds"] == rec.SEEDS
    assert doc["paths"] == rec.PATHS and doc["calls"] == list(rec.CALLS)
    return doc["cases"]


@pytest.mark.parametrize("path", list(rec.PATHS))
@pytest.mark.parametrize("name", rec.MESHES)
def test_paths_equal_the_recorded_bits(golden, name, path):
    got, want = rec.record(name, path), golden[name][rec.PATHS[path]]   # (record asserts two colours or more, and lat30's colour width)
    for what in rec.WHAT:
        if not isinstance(want[what], list):
            assert got[what] == want[what], (name, path, what, got[what], want[what])
            continue
        bad = [i for i, (g, w) in enumerate(zip(got[what], want[what])) if g != w]
        assert len(got[what]) == len(want[what]) and bad == [], (name, path, what, len(bad), [(i, got[what][i], want[what][i]) for i in bad[:2]])
