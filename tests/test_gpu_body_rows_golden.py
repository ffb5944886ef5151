"""The per-body rows bit for bit against tests/golden/body_rows_bits.json, recorded by tools/record_body_rows.py from the build whose
source_sha the file names: the observation's sums and the pose's raw moments are elsewhere compared against bounds from exact arithmetic,
which a reordered reduction tree would pass.  The cases, their seeded states and the recording itself are the tool's (imported here), so
the file and the test cannot drift apart.  The rows come from the rows in the caller's numbering, so both kinds of body give the one
golden.  The file is never recorded again: a difference is a change of the reduction order, of a chunk's cut or of the arithmetic."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_body_rows", os.path.join(ROOT, "tools", "record_body_rows.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        doc = json.load(f)
    assert sorted(doc["cases"]) == sorted(rec.CASES) and doc["seeds"] == rec.SEEDS and doc["kinds"] == list(rec.KINDS)
    return doc["cases"]


@pytest.mark.parametrize("kind", list(rec.KINDS))
@pytest.mark.parametrize("name", rec.CASES)
def test_rows_equal_the_recorded_bits(golden, name, kind):
    got, want = rec.record(name, kind), golden[name]
    assert sorted(got) == sorted(want)
    for what in want:
        bad = [b for b, (g, w) in enumerate(zip(got[what], want[what])) if g != w]
        assert len(got[what]) == len(want[what]) and bad == [], (name, kind, what, bad, [(got[what][b], want[what][b]) for b in bad[:2]])


@pytest.mark.parametrize("kind", list(rec.KINDS))
def test_a_body_of_the_mixed_batch_alone_gives_the_recorded_bits(golden, kind):
    """the promise the shared reduction exists to keep: a body of a batch gives the bits it gives alone -- here against the batch's golden"""
    parts, pos, vel, _ = rec.case("mixed")
    first = np.concatenate([[0], np.cumsum([len(v) for v, _ in parts])])
    for b, part in enumerate(parts):
        solo = rec.make([part], kind)
        solo.writeState(pos[first[b]:first[b + 1]], vel[first[b]:first[b + 1]])
        for what, rows in (("observations", solo.bodyObservations()), ("poses", solo.bodyPoses())):
            assert rec.hex_rows(rows, np.float64) == golden["mixed"][what][b:b + 1], (kind, b, what)
        solo.close()
