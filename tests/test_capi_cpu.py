"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/tetsim.h declares, refuses to
compute without a GPU (no fallback), and its host preprocessing matches the reference-pinned data."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_f32, load_mesh
from oracle import OraclePJ
from tetsim_amd import _capi as capi
from tetsim_amd import make_lattice

ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "tetsim.h")).read()
    declared = sorted(set(re.findall(r"\b(tetsim_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(capi.SYMBOLS)
    L = capi.lib()
    for s in declared:
        assert hasattr(L, s), s
    assert L.tetsim_abi_version() == 5


def test_library_info_matches_the_tree():
    """The loaded library says which sources it was built from; the product build is never the ablation build."""
    from tetsim_amd.build import source_shas
    info = capi.library_info()
    assert info["abi"] == 5 and info["ablation"] is False
    assert (info["source_sha"], info["kernel_sha"]) == source_shas(), "libtetsim_hip.so is stale: run python -m tetsim_amd.build"
    assert re.fullmatch(r"[0-9a-f]{16}", info["source_sha"]) and re.fullmatch(r"[0-9a-f]{16}", info["kernel_sha"])


def test_library_info_names_the_environment_knobs_it_sees():
    """debug_env is a bit mask on the C side and a list of names in Python: the two tables must stay in step."""
    import subprocess
    import sys
    code = "import json; from tetsim_amd import _capi; print(json.dumps(_capi.library_info()['debug_env']))"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clean = {k: v for k, v in os.environ.items() if k not in capi.DEBUG_ENV_NAMES}
    assert json.loads(subprocess.run([sys.executable, "-c", code], cwd=root, env=clean, capture_output=True, text=True, check=True).stdout) == []
    for name in capi.DEBUG_ENV_NAMES:
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(clean, **{name: "1"}), capture_output=True, text=True, check=True).stdout
        # (the product library neither reads nor reports the A/B switches of settled choices: development build only)
        assert json.loads(out) == ([] if name in capi.LAB_ENV_NAMES else [name]), (name, out)
    blob = open(capi.LIB_PATH, "rb").read()
    for name in capi.DEBUG_ENV_NAMES:   # the product binary does not even contain the names it does not read
        assert (name.encode() in blob) == (name not in capi.LAB_ENV_NAMES), name


def test_product_kernel_has_no_ablation_knobs():
    """TETSIM_DEBUG_ITERS & co. exist only in the -DTETSIM_ABLATION build: the product binary does not even contain the names, and the
    product's kernel sources have no `#ifdef TETSIM_ABLATION` and no getenv left (the laboratory lives in pj_lab.h / pj_blocked_lab.inc)."""
    blob = open(capi.LIB_PATH, "rb").read()
    for name in (b"TETSIM_DEBUG_ITERS", b"TETSIM_DEBUG_SKIP_REST_STORE", b"TETSIM_DEBUG_NO_PEEL", b"TETSIM_DEBUG_STAGGER", b"TETSIM_DEBUG_ITER_HIST"):
        assert name not in blob, name
    src = os.path.join(os.path.dirname(capi.LIB_PATH), "csrc")
    for f in ("pj_blocked.hip", "pj_math.inc"):
        text = open(os.path.join(src, f)).read()
        assert "#ifdef TETSIM_ABLATION" not in text and "defined(TETSIM_ABLATION" not in text and "getenv" not in text, f


def test_no_cpu_fallback():
    """Without a HIP device create must FAIL loudly (ENODEVICE); with one it must succeed on the GPU."""
    L = capi.lib()
    v, t = make_lattice(2)
    v = np.ascontiguousarray(v.reshape(-1)); t = np.ascontiguousarray(t.reshape(-1))
    h = C.c_void_p()
    rc = L.tetsim_create(fp(v), len(v) // 3, ip(t), len(t) // 4, None, C.byref(h))
    if rc == capi.OK:
        L.tetsim_destroy(h)
        pytest.skip("a GPU is present; the failure path is exercised on CPU-only hosts")
    assert rc == capi.ENODEVICE and not h.value
    assert b"no CPU fallback" in L.tetsim_last_error(None)


def test_invalid_meshes_are_rejected():
    L = capi.lib()
    v, t = make_lattice(2)
    v = np.ascontiguousarray(v.reshape(-1)); t = np.ascontiguousarray(t.reshape(-1)).copy()
    t[5] = 10 ** 6
    h = C.c_void_p()
    assert L.tetsim_create(fp(v), len(v) // 3, ip(t), len(t) // 4, None, C.byref(h)) == capi.EINVAL
    assert b"outside" in L.tetsim_last_error(None)
    lv = np.zeros(len(t) // 4, dtype=np.int32); n = C.c_uint32()
    assert L.tetsim_prep_levels(ip(t), len(t) // 4, len(v) // 3, ip(lv), C.byref(n)) == capi.EINVAL


@pytest.mark.parametrize("mesh", ["dragon", "lat4", "lat4c", "lat2degen"])
def test_prep_rest_bit_exact_vs_reference(mesh):
    """tetsim_prep_rest (product code) against arrays recorded from the reference's initPhysics."""
    L = capi.lib()
    v, t = load_mesh(mesh)
    v = np.ascontiguousarray(v.reshape(-1)); t = np.ascontiguousarray(t.reshape(-1))
    nv, nt = len(v) // 3, len(t) // 4
    im, irp, irv = np.empty(nv, np.float32), np.empty(9 * nt, np.float32), np.empty(nt, np.float32)
    assert L.tetsim_prep_rest(fp(v), nv, ip(t), nt, 1000.0, fp(im), fp(irp), fp(irv)) == 0
    assert np.array_equal(im.view(np.uint32), load_f32(mesh + "_invMass.f32").view(np.uint32))
    assert np.array_equal(irp.view(np.uint32), load_f32(mesh + "_invRestPose.f32").view(np.uint32))
    assert np.array_equal(irv.view(np.uint32), load_f32(mesh + "_invRestVolume.f32").view(np.uint32))


# The 3-cell lattice at this density gives its eight inner particles the inverse mass 0x3F800009 = 1 + 65,536 x 0x3F80 + 8: the stamp the
# clustered FAST Neo-Hookean call kernel (8 colours) waits for in prev.w at substep 2 of the call whose block is 0x3F80 -- the 16,256th
# tetsim_step_n call of the body (next_epoch_block: frame_epoch = 1 + 65,536 x calls; stamps of substep s are frame_epoch + 8 s + colour,
# and substep 2's first touchers look for frame_epoch + 8 in prev.w).  tests/test_gpu_nh_one_launch_irregular.py runs through it.
STAMP_DENSITY = 26.99997
STAMP_BITS = 0x3F800009


def test_stamp_density_gives_the_colliding_inverse_mass():
    L = capi.lib()
    v, t = make_lattice(3, y0=0.3)
    vv, tt = np.ascontiguousarray(v.ravel()), np.ascontiguousarray(t.ravel().astype(np.int32))
    nv, nt = len(v), len(t)
    im, irp, irv = np.empty(nv, np.float32), np.empty(9 * nt, np.float32), np.empty(nt, np.float32)
    assert L.tetsim_prep_rest(fp(vv), nv, ip(tt), nt, STAMP_DENSITY, fp(im), fp(irp), fp(irv)) == 0
    hit = np.flatnonzero(im.view(np.uint32) == STAMP_BITS)
    inner = [i + 4 * (j + 4 * k) for k in (1, 2) for j in (1, 2) for i in (1, 2)]
    assert hit.tolist() == inner
    out = [np.full(nt, -1, np.int32) for _ in range(4)]
    nl, nc = C.c_uint32(), C.c_uint32()
    assert L.tetsim_prep_clusters(ip(tt), nt, nv, *[ip(a) for a in out], C.byref(nl), C.byref(nc)) == 0
    assert nl.value == 8 and nc.value == 27 and np.unique(t).size == nv          # the call kernel's body: 2..127 colours, no free particle
    calls = 16256
    assert 1 + 65536 * calls + 8 == STAMP_BITS


def _py_levels(t, nv):
    last = np.full(nv, -1, dtype=np.int64)
    out = np.empty(len(t), dtype=np.int32)
    for e, tet in enumerate(t.tolist()):
        l = max(last[x] for x in tet) + 1
        out[e] = l
        for x in tet:
            last[x] = l
    return out


@pytest.mark.parametrize("mesh", ["dragon", "lat4"])
def test_levels_and_colours(mesh):
    L = capi.lib()
    v, t = load_mesh(mesh)
    tf = np.ascontiguousarray(t.reshape(-1))
    nv, nt = len(v), len(t)
    lv, n = np.empty(nt, np.int32), C.c_uint32()
    assert L.tetsim_prep_levels(ip(tf), nt, nv, ip(lv), C.byref(n)) == 0
    assert np.array_equal(lv, _py_levels(t, nv)) and n.value == lv.max() + 1
    # tets of one level are vertex-disjoint; sharing pairs keep their order
    for l in range(n.value):
        ids = t[lv == l].ravel()
        assert len(np.unique(ids)) == len(ids)
    col, nc = np.empty(nt, np.int32), C.c_uint32()
    assert L.tetsim_prep_colours(ip(tf), nt, nv, ip(col), C.byref(nc)) == 0
    for c in range(nc.value):
        ids = t[col == c].ravel()
        assert len(np.unique(ids)) == len(ids)
    assert nc.value <= np.bincount(t.ravel()).max() * 4  # greedy bound: deg + 1
    # colour-sorting then levelling gives at most nc levels
    order = np.argsort(col, kind="stable")
    ts = np.ascontiguousarray(t[order].reshape(-1))
    assert L.tetsim_prep_levels(ip(ts), nt, nv, ip(lv), C.byref(n)) == 0
    assert n.value <= nc.value


@pytest.mark.parametrize("quirk", [0, 1])
@pytest.mark.parametrize("mesh", ["dragon", "lat4"])
def test_slot_table_matches_oracle(mesh, quirk):
    """Product table builder vs the oracle's direct emulation of SoftbodyGPU.js:563-577."""
    L = capi.lib()
    v, t = load_mesh(mesh)
    tf = np.ascontiguousarray(t.reshape(-1))
    slots, dropped = np.empty(len(v) * 36, np.int32), C.c_uint32()
    assert L.tetsim_prep_slot_table(ip(tf), len(t), len(v), quirk, ip(slots), C.byref(dropped)) == 0
    orc = OraclePJ(v, t, {"density": 1000.0}, slot_quirk=bool(quirk))
    assert np.array_equal(slots.reshape(-1, 36), orc.slots)
    assert dropped.value == quirk  # the only loss on these meshes is tet 0 / corner 0
    if mesh == "dragon":
        assert orc.biggestT == 7  # SURVEY.md §8(a) G1 probe: highest table used on the Dragon


def test_tolerance_table_obeys_the_three_times_rule():
    """tests/golden/tolerances.json (calibrated on MI355X): every check's allowed error is at most 3 x the error observed when it
    was calibrated, never above the bound its test states, and bit-identical checks (observed 0) carry
    an ulp-level bound.  conftest.within() enforces the table."""
    import json
    from conftest import GOLDEN, within
    with open(os.path.join(GOLDEN, "tolerances.json")) as f:
        tab = json.load(f)["checks"]
    assert len(tab) > 200
    for label, c in tab.items():
        assert 0.0 < c["allowed"] <= c["stated"] * (1 + 1e-12), label
        if c.get("contract") is False:
            assert c["allowed"] == c["stated"] and len(c["why"]) > 40, label   # a report row: stated bound only, and says why
        elif c["observed"] > 0.0:
            assert c["allowed"] <= 3.0 * c["observed"] * (1 + 1e-9), (label, c)
        else:
            assert c["allowed"] <= 1e-6, (label, c)
    label, c = next((k, v) for k, v in tab.items() if v["observed"] > 0 and v["allowed"] < v["stated"])
    within(label, c["allowed"], c["stated"])                       # at the calibrated bound: passes
    with pytest.raises(AssertionError, match="allowed"):
        within(label, c["allowed"] * 1.01, c["stated"])             # 1% above it: fails although far below the stated bound


# sha256 over "label\tceiling\n" of the ceilings frozen in rounds 3 and 4, in file order (tools/tolerance_freeze.py re-derives the
# file from commits 57b715d / e2f084b).  Editing a frozen ceiling turns this red; later rounds only APPEND labels.
FROZEN_CEILINGS_SHA256 = "849354966fba9e96ff89d52c9a565b6faf8a671e6155ab847355af68e8cf8eab"


def test_tolerance_table_is_frozen_and_only_ratchets_down():
    """the parity contract must not move with the implementation.  Every label has a ceiling in
    tests/golden/tolerance_ceilings.json; the table may allow more than a label's ceiling only on a row whose "reason" names
    the commit and the cause; the ceilings recorded in rounds 3 / 4 are pinned by digest; a report row ("contract": false)
    is not a way around it (the two 600-substep velocity rows are the only ones); within() enforces the ceiling even if the
    table were edited by hand; tools/tolerance_report.py refuses a calibration run that drifted above a ceiling."""
    import hashlib
    import json
    import re
    import conftest
    from conftest import GOLDEN, within
    with open(os.path.join(GOLDEN, "tolerances.json")) as f:
        tab = json.load(f)["checks"]
    with open(os.path.join(GOLDEN, "tolerance_ceilings.json")) as f:
        ceil = json.load(f)["ceilings"]
    assert set(tab) - set(k for k, c in tab.items() if c.get("contract") is False) <= set(ceil), set(tab) - set(ceil)
    frozen = [(k, c) for k, c in ceil.items() if c["since"].startswith(("round 3", "round 4"))]
    assert len(frozen) == 277 and sum(c["since"].startswith("round 3") for _, c in frozen) == 264
    digest = hashlib.sha256("".join("%s\t%r\n" % (k, c["ceiling"]) for k, c in frozen).encode()).hexdigest()
    assert digest == FROZEN_CEILINGS_SHA256, digest
    above, reports = [], []
    for label, c in tab.items():
        if c.get("contract") is False:
            reports.append(label)
            continue
        if c["allowed"] > ceil[label]["ceiling"]:
            above.append(label)
            assert re.search(r"commit [0-9a-f]{7}", c.get("reason", "")) and len(c["reason"]) > 60, (label, "above its ceiling without a reason")
            assert c["observed"] > ceil[label]["ceiling"], (label, "a reason is for an error that left the ceiling, not for slack")
    assert len(above) <= 12, above                                   # reasons are exceptions, not the rule (4 at the freeze)
    assert sorted(reports) == ["polar fast gather vs reference GLSL dragon @600 (vel)", "polar fast vs reference GLSL dragon @600 (vel)"]
    # within() itself holds the ceiling: a hand-edited table row without a reason does not buy slack
    label = next(k for k, c in tab.items() if c.get("contract") is not False and "reason" not in c and c["allowed"] < c["stated"] / 4)
    saved = dict(conftest._tol_table()[label])
    try:
        conftest._tol_table()[label]["allowed"] = saved["stated"]
        with pytest.raises(AssertionError, match="allowed"):
            within(label, ceil[label]["ceiling"] * 1.01, saved["stated"])
        within(label, ceil[label]["ceiling"], saved["stated"])
    finally:
        conftest._tol_table()[label].update(saved)


def test_tolerance_report_refuses_to_loosen_silently():
    """tools/tolerance_report.py: a calibration run whose observed error exceeds a frozen ceiling is refused unless a reason
    is given; 3 x a larger-but-still-under-the-ceiling error is capped at the ceiling; new labels get a ceiling."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import tolerance_report as tr
    table = {"a": {"observed": 1e-6, "allowed": 3e-6, "stated": 1e-3}, "b": {"observed": 1e-6, "allowed": 3e-6, "stated": 1e-3},
             "r": {"observed": 0.2, "allowed": 24.0, "stated": 24.0, "contract": False, "why": "chaos"}}
    ceilings = {"a": {"ceiling": 3e-6, "since": "round 3"}, "b": {"ceiling": 3e-6, "since": "round 3"}}
    rows = {"a": {"observed": 2e-6, "allowed": 1e-3}, "b": {"observed": 4e-6, "allowed": 1e-3}, "r": {"observed": 0.9, "allowed": 24.0},
            "new": {"observed": 5e-7, "allowed": 1e-3}}
    out, ceil, refused = tr.merge(rows, table, {k: dict(v) for k, v in ceilings.items()}, {}, "round 5")
    assert [k for k, _, _ in refused] == ["b"]                      # drifted above its ceiling, no reason
    assert out["a"]["allowed"] == 3e-6 and "reason" not in out["a"]  # 3 x 2e-6 would be 6e-6: capped at the ceiling
    assert out["r"]["contract"] is False and out["r"]["allowed"] == 24.0
    assert dict(ceil["new"]) == {"ceiling": 1.5e-6, "since": "round 5"} and ceil["a"]["ceiling"] == 3e-6
    out, ceil, refused = tr.merge(rows, table, {k: dict(v) for k, v in ceilings.items()}, {"b": "commit 1234567: why"}, "round 5")
    assert not refused and out["b"]["allowed"] == 1.2e-5 and out["b"]["reason"].startswith("commit 1234567")
    assert ceil["b"]["ceiling"] == 3e-6                             # a reason never raises the ceiling itself
