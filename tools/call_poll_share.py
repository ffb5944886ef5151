#!/usr/bin/env python3
"""Where the one-launch polar call's workgroups spend their residency: looking, or working.  1 M-tet lattice on the floor, development build
(python -m tetsim_amd.build --ablation; TETSIM_DEBUG_POLL_TRACE, pj_lab.h): the first wave of every workgroup of the substep in the MIDDLE
of a call stamps its start, its first look, its last successful look and its end, and counts its looks.

    python tools/call_poll_share.py run DIR [lag ...]       one child process per lag (needs the GPU): DIR/poll_lag<L>.bin
    python tools/call_poll_share.py report DIR [lag ...]    host only: the tables of profiles/r07_call_poll_share.txt

Per lag: for tile blocks and particle blocks the share of resident time between the first look issued and the last look succeeded, the
looks per block by position in the substep (tenths of the table's tile / particle entries), and the tiles at the START of an XCD's range
whose predictions come from particle blocks fed by tiles that are dispatched much later in the substep (another XCD's range end)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELLS, SUB, DT = 55, 20, (1.0 / 60.0) / 20
PP = dict(gravity=-9.81, friction=1000.0, density=1000.0, devCompliance=1e-5, volCompliance=0.0, worldBounds=[-2.5, -1.0, -2.5, 2.5, 10.0, 2.5])


def child(lag):
    import time
    from tetsim_amd import SoftBodyHIP, make_lattice
    v, t = make_lattice(CELLS)
    b = SoftBodyHIP(v, t, None, dict(PP), solver="polar", precision="fast")
    assert b.info.fused_particle_pass == 5
    for _ in range(45):                      # the body reaches the floor around frame 19 and settles
        b.simulateSubsteps(SUB, DT, PP)
    b.sync()
    t0 = time.perf_counter()
    for _ in range(10):
        b.simulateSubsteps(SUB, DT, PP)
    b.sync()
    print("lag %d: %.2f us per substep on the floor (development build, stamps on)" % (lag, (time.perf_counter() - t0) / (10 * SUB) * 1e6), flush=True)
    b.close()                                # (the trace is written as the body goes)
    return 0


def run(out, lags):
    os.makedirs(out, exist_ok=True)
    for lag in lags:
        env = dict(os.environ, TETSIM_HIP_LIB=os.path.join(ROOT, "tetsim_amd", "libtetsim_hip_ablation.so"), TETSIM_PJ_CALL_LAG=str(lag),
                   TETSIM_DEBUG_POLL_TRACE=os.path.join(out, "poll_lag%d.bin" % lag))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(lag)], env=env, timeout=240)
        if r.returncode != 0:                # (nothing more on the GPU behind a failure)
            print("lag %d: the child ended with %d" % (lag, r.returncode))
            return 1
    return 0


def tenths(pos, cols, names, fmt):
    order = np.argsort(pos)
    print("    tenth of the entries |      n | " + " ".join("%12s" % x for x in names))
    for q, part in enumerate(np.array_split(order, 10)):
        print("    %20d | %6d | " % (q + 1, len(part)) + " ".join(f % c[part].mean() for f, c in zip(fmt, cols)))


def report(out, lags):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_call_schedule import Tiles
    from tetsim_amd import make_lattice
    v, t = make_lattice(CELLS)
    T = Tiles(v, t)
    nb, npb, per = T.nb, T.npb, T.per_xcd
    print("lattice %d^3 cells: %d tiles (%d per XCD), %d particle blocks; times in s_memtime ticks of the workgroup's own XCD (the XCDs' counters are not synchronised: differences inside a workgroup only)" % (CELLS, nb, per, npb))
    # tiles whose predictions hang on tiles dispatched much later in the substep: walk index of the latest tile on the lists of the
    # particle blocks a tile stages, minus its own walk index (a tile's walk index is its row in its XCD's range)
    walk = np.arange(nb) % per
    reach = np.array([max(int(walk[b2]) for k in T.pbs_of_tile[b] for b2 in T.tiles_of_pb[k]) for b in range(nb)])
    other = np.array([any(b2 // per != b // per for k in T.pbs_of_tile[b] for b2 in T.tiles_of_pb[k]) for b in range(nb)])
    ahead = reach - walk
    late = other & (ahead >= per // 2)
    print("tiles that stage a particle whose block waits for a tile of ANOTHER XCD's range: %d of %d; of those, the tile they wait for (through the "
          "particle block) is dispatched >= half a range (%d rows) after their own row: %d, all within the first %d rows of their range"
          % (other.sum(), nb, per // 2, late.sum(), (walk[late].max() + 1) if late.any() else 0))
    print("  rows ahead (latest tile it depends on, minus its own row), every tile: median %d, 90%% %d, max %d" % (np.median(ahead), np.percentile(ahead, 90), ahead.max()))
    for lag in lags:
        tr = np.fromfile(os.path.join(out, "poll_lag%d.bin" % lag), dtype=np.uint64).reshape(-1, 8).astype(np.int64)
        assert len(tr) == 2 * nb + npb
        entry, period, tail, fell, why = T.schedule(lag)
        tl, pb = tr[nb:2 * nb], tr[2 * nb:]
        assert (tl[:, 4] > 0).all() and (pb[:, 4] > 0).all(), "every block of the middle substep left its row"
        print("\n== lag %d: period %d, tail %d%s ==" % (lag, period, tail, " (FELL BACK: %s)" % why if fell else ""))
        res, wave, blk, looks = tl[:, 4] - tl[:, 0], tl[:, 2] - tl[:, 1], tl[:, 3] - tl[:, 1], tl[:, 5]
        print("  TILE blocks: resident %.0f ticks on average; first look issued -> every wave's last look succeeded %.0f (share %.3f); first wave alone %.0f (share %.3f); "
              "looks of the first wave %.2f on average, max %d, one look sufficed in %.1f %% of the tiles"
              % (res.mean(), blk.mean(), blk.sum() / res.sum(), wave.mean(), wave.sum() / res.sum(), looks.mean(), looks.max(), 100.0 * (looks == 1).mean()))
        tenths(tl[:, 6] % period, (res, blk, blk / res, looks), ("resident", "looking", "share", "looks"), ("%12.0f", "%12.0f", "%12.3f", "%12.2f"))
        print("  tiles at the start of an XCD's range that wait for another range's end (%d tiles): looking %.0f ticks on average, share %.3f, looks %.2f; every other tile: %.0f, %.3f, %.2f"
              % (late.sum(), blk[late].mean(), blk[late].sum() / res[late].sum(), looks[late].mean(), blk[~late].mean(), blk[~late].sum() / res[~late].sum(), looks[~late].mean()))
        res, sums, allp, looks = pb[:, 4] - pb[:, 0], pb[:, 2] - pb[:, 1], pb[:, 3] - pb[:, 1], pb[:, 5]
        print("  PARTICLE blocks (first wave of four): resident %.0f ticks on average; first look issued -> every sum stamped %.0f (share %.3f); -> previous position stamped too %.0f "
              "(share %.3f); looks %.2f on average, max %d, one look sufficed in %.1f %% of the blocks"
              % (res.mean(), sums.mean(), sums.sum() / res.sum(), allp.mean(), allp.sum() / res.sum(), looks.mean(), looks.max(), 100.0 * (looks == 1).mean()))
        tenths(pb[:, 6] % period + period * (pb[:, 6] % period < tail), (res, allp, allp / res, looks), ("resident", "looking", "share", "looks"),
               ("%12.0f", "%12.0f", "%12.3f", "%12.2f"))
        # slot time: a workgroup holds one of the chip's 2,048 slots while it is resident
        tile_slot, pb_slot = (tl[:, 4] - tl[:, 0]).sum(), (pb[:, 4] - pb[:, 0]).sum()
        print("  slot time of the substep: tiles %d ticks, particle blocks %d (%.1f %% of the sum); looking: tiles %d (%.1f %%), particle blocks %d (%.1f %%)"
              % (tile_slot, pb_slot, 100.0 * pb_slot / (tile_slot + pb_slot), blk.sum(), 100.0 * blk.sum() / (tile_slot + pb_slot), allp.sum(), 100.0 * allp.sum() / (tile_slot + pb_slot)))
    return 0


if __name__ == "__main__":
    mode, out = sys.argv[1], sys.argv[2]
    if mode == "child":
        sys.exit(child(int(out)))
    lags = [int(x) for x in sys.argv[3:]] or [0, 16, 128]
    sys.exit(run(out, lags) if mode == "run" else report(out, lags))
