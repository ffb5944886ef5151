"""The blocked polar kernels bit for bit against tests/golden/polar_bits/*.npy, recorded by tools/record_polar_bits.py from the build the
directory's SOURCE file names -- the build BEFORE the tiles' reduction went from gathering through an index table to summing runs of a
list (host_prep.h: tet_pos, lc_first).  A tile adds the same addends in the same order, so every position, velocity and quaternion keeps
its bits: on the persistent frame kernel and the fused kernel (the irregular body), on the one-launch call and the kernel pair (the same
body with a loose particle; the 45-cell lattice), for the carried record, the lean record and the constant rest shape.  The cases, their
meshes and the stepping are the tool's (imported here), so the files and the test cannot drift apart; what makes the meshes hard --
ragged tiles, runs of every length mod 4, dropped corners, particles in nine tiles -- is asserted on the host in tests/test_tile_tables.py.
The files are never recorded again: a difference is a change of the reduction order or of the arithmetic."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_polar_bits", os.path.join(ROOT, "tools", "record_polar_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

# TetSimInfo.fused_particle_pass: 2 = a call is one persistent launch of 256-tet tiles (tetsim_step: the fused kernel), 5 = a call is one
# launch of tiles and particle blocks (tetsim_step: the tet kernel + particle kernel pair)
PATH = {"irregular": 2, "loose": 5, "lattice": 5}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("stepper", ["step_n", "step"])
@pytest.mark.parametrize("flag", list(rec.FLAGS))
@pytest.mark.parametrize("case", rec.CASES)
def test_forty_substeps_equal_the_recorded_bits(case, flag, stepper):
    got, path = rec.run(case, flag, stepper)
    assert path == PATH[case], (case, flag, path)
    for field in rec.FIELDS:
        want = np.load(rec.path_of("%s_%s_%s" % (case, flag, field)))
        have = rec.sample(got[field])
        assert have.shape == want.shape and want.dtype == np.float32, (case, flag, field)
        bad = np.nonzero((_bits(have) != _bits(want)).any(axis=1))[0]
        assert bad.size == 0, (case, flag, stepper, field, bad.size, bad[:4].tolist(), have[bad[:2]].tolist(), want[bad[:2]].tolist())
