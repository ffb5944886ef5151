"""The dispatch table of the one-launch polar call (host_prep.cpp: build_call_schedule, through tetsim_prep_call_schedule): host only.

Block g of a call runs entry g % period for substep g / period, one less for a wrapped entry.  The call makes progress if whatever a
block waits for has a smaller grid index.  That is checked HERE, in Python, from the tiles' particle lists and the particles' tile lists --
not by asking the builder's own checker, which is only cross-checked at the end."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_call_kernel_irregular import _loose
from tetsim_amd import _capi as capi, make_lattice

u32p = C.POINTER(C.c_uint32)
NONE = 0xFFFFFFFF
TILE, PARTICLES, EMPTY = 0, 1, 2


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Tiles:
    """What the table is built from, for a mesh tiled as an unpartitioned body is."""

    def __init__(self, v, t):
        L = capi.lib()
        vv, tt = np.ascontiguousarray(v, np.float32).ravel(), np.ascontiguousarray(t, np.int32).ravel()
        sizes = np.zeros(4, np.uint32)
        args = (_ptr(vv, C.c_float), len(vv) // 3, _ptr(tt, C.c_int32), len(tt) // 4, _ptr(sizes, C.c_uint32))
        assert L.tetsim_prep_call_tiles(*args, None, None, None) == 0
        self.nb, slots, self.vp_cols, self.nv_pad = (int(x) for x in sizes)
        self.nv = len(vv) // 3
        self.off = np.zeros(self.nb + 1, np.uint32)
        self.verts = np.zeros(slots, np.int32)
        self.ell = np.zeros(self.vp_cols * self.nv_pad, np.uint32)
        assert L.tetsim_prep_call_tiles(*args, _ptr(self.off, C.c_uint32), _ptr(self.verts, C.c_int32), _ptr(self.ell, C.c_uint32)) == 0
        self.per_xcd = (self.nb + 7) // 8
        self.tet_blocks = 8 * self.per_xcd
        self.npb = (self.nv + 255) // 256
        self.plain_period = (self.tet_blocks + self.npb + 7) & ~7
        # per particle block the tiles on its particles' lists; per tile the particle blocks that own what it stages
        ell = self.ell.reshape(self.vp_cols, self.nv_pad)[:, :self.nv]
        col, v_of = np.nonzero(ell != NONE)
        tile_of_slot = np.searchsorted(self.off, ell[col, v_of], side="right") - 1
        self.tiles_of_pb = [set() for _ in range(self.npb)]
        for k, b in zip(v_of // 256, tile_of_slot):
            self.tiles_of_pb[k].add(int(b))
        self.pbs_of_tile = [set(int(x) // 256 for x in self.verts[self.off[b]:self.off[b + 1]]) for b in range(self.nb)]
        self.longest_list = int((ell != NONE).sum(axis=0).max())

    def _args(self):
        return (_ptr(self.verts, C.c_int32), _ptr(self.off, C.c_uint32), self.nb, _ptr(self.ell, C.c_uint32), self.vp_cols, self.nv_pad, self.nv)

    def schedule(self, lag):
        L = capi.lib()
        period, tail, fell = C.c_uint32(), C.c_uint32(), C.c_int32(-1)
        assert L.tetsim_prep_call_schedule(*self._args(), lag, None, 0, C.byref(period), C.byref(tail), C.byref(fell)) == 0
        entry = np.zeros(period.value, np.uint32)
        assert L.tetsim_prep_call_schedule(*self._args(), lag, _ptr(entry, C.c_uint32), len(entry) - 1, C.byref(period), C.byref(tail), None) != 0   # too little room
        assert L.tetsim_prep_call_schedule(*self._args(), lag, _ptr(entry, C.c_uint32), len(entry), C.byref(period), C.byref(tail), C.byref(fell)) == 0
        why = L.tetsim_last_error(None).decode() if fell.value else ""
        return entry, period.value, tail.value, bool(fell.value), why

    def builder_check(self, entry, period, tail):
        e = np.ascontiguousarray(entry, np.uint32)
        return capi.lib().tetsim_prep_check_call_schedule(*self._args(), _ptr(e, C.c_uint32), period, tail)

    def plain(self):
        e = np.full(self.plain_period, EMPTY << 30, np.uint32)
        for r in range(self.tet_blocks):
            if (r & 7) * self.per_xcd + (r >> 3) < self.nb:
                e[r] = TILE << 30 | r
        e[self.tet_blocks:self.tet_blocks + self.npb] = (PARTICLES << 30) | np.arange(self.npb, dtype=np.uint32)
        return e


def _check(T, entry, period, tail):
    """The table's completeness, its tiles' placement and the four orderings, entry by entry."""
    assert period % 8 == 0 and period >= T.plain_period and len(entry) == period and 0 <= tail <= period
    kind, wrapped, index = entry >> 30, (entry >> 29) & 1, entry & ((1 << 29) - 1)
    assert set(np.unique(kind)) <= {TILE, PARTICLES, EMPTY}
    pos = np.arange(period)
    # tiles: each exactly once, on its XCD, every XCD walking its eighth in order, never wrapped
    tp, tr = pos[kind == TILE], index[kind == TILE].astype(np.int64)
    tile = (tr & 7) * T.per_xcd + (tr >> 3)
    assert sorted(tile) == list(range(T.nb))
    assert np.array_equal(tr & 7, tp & 7) and not wrapped[kind == TILE].any()
    for x in range(8):
        rows = tr[(tr & 7) == x] >> 3
        assert np.all(np.diff(rows) > 0), x
    # particle blocks: each exactly once; wrapped ones inside the tail
    pp, pk, pw = pos[kind == PARTICLES], index[kind == PARTICLES], wrapped[kind == PARTICLES]
    assert sorted(pk) == list(range(T.npb))
    assert not pw.any() or tail >= pp[pw == 1].max() + 1
    assert pw.any() or tail == 0
    # where everything of substep 0 sits in the grid (a wrapped entry one period on); substep s is s periods further
    at_tile = np.empty(T.nb, np.int64)
    at_tile[tile] = tp
    at_pb = np.empty(T.npb, np.int64)
    at_pb[pk] = pp + period * pw.astype(np.int64)
    for k in range(T.npb):
        for b in T.tiles_of_pb[k]:
            assert at_tile[b] < at_pb[k], ("a tile of s on a particle block's lists precedes that block", b, k)
    for b in range(T.nb):
        for k in T.pbs_of_tile[b]:
            assert at_pb[k] < at_tile[b] + period, ("a particle block of s precedes the tile of s + 1 that stages its particles", k, b)
    # (block k of s precedes block k of s + 1, tile b of s precedes tile b of s + 1: by construction, not by a test -- every block has exactly
    # one entry per period, asserted above, so its entries of consecutive substeps are one period apart)
    return at_tile, at_pb


_cache = {}


def _body(name):
    if name not in _cache:
        if name == "lattice12":
            v, t = make_lattice(12, y0=0.01)
        else:
            v, t = _loose(*{"loose31": (31, 2302), "loose33": (33, 4096)}[name])
        _cache[name] = Tiles(v, t)
    return _cache[name]


BODIES = ["lattice12", "loose31", "loose33"]


@pytest.mark.parametrize("name", BODIES)
def test_the_inputs_are_what_the_test_means_them_to_be(name):
    T = _body(name)
    assert T.nb > 8 and T.npb > 1
    if name != "lattice12":
        assert T.longest_list > 9, "irregular bodies: particle lists longer than nine"
    for b in range(T.nb):                                            # every tile that stages a particle is on that particle's lists
        for k in T.pbs_of_tile[b]:
            assert b in T.tiles_of_pb[k]


@pytest.mark.parametrize("name", BODIES)
@pytest.mark.parametrize("lag", [0, 1, 3, "more than the tiles"])
def test_every_table_keeps_the_progress_invariant(name, lag):
    T = _body(name)
    L = T.nb + 1 if lag == "more than the tiles" else lag
    entry, period, tail, fell, why = T.schedule(L)
    at_tile, at_pb = _check(T, entry, period, tail)
    assert T.builder_check(entry, period, tail) == 0
    if L == 0:
        assert not fell and tail == 0 and np.array_equal(entry, T.plain()), "lag 0 is today's [tiles | particles] order"
    elif L > T.nb:
        assert fell and "lag %d" % L in why and np.array_equal(entry, T.plain()), "a lag of a whole substep falls back and says so"
    elif not fell:
        # the lag itself: an unwrapped particle block sits at least 8 * L behind the last tile on its lists
        wrapped = at_pb >= period
        for k in range(T.npb):
            if T.tiles_of_pb[k] and not wrapped[k]:
                assert at_pb[k] >= max(at_tile[b] for b in T.tiles_of_pb[k]) + 8 * L, k
        assert not np.array_equal(entry, T.plain())
    else:
        assert why and np.array_equal(entry, T.plain())


def test_the_checker_refuses_tables_that_could_hang():
    """Cross-check of the builder's own checker (what tetsim_create relies on): it passes what the Python check passes and refuses a
    table with a particle block in front of one of its tiles, a tile off its XCD, a missing or doubled block, a tail that is too short."""
    T = _body("lattice12")
    entry, period, tail, fell, _ = T.schedule(1)
    assert not fell and T.builder_check(entry, period, tail) == 0
    plain = T.plain()
    assert T.builder_check(plain, T.plain_period, 0) == 0
    bad = plain.copy()                                               # the first particle block in front of every tile
    first_pb = T.tet_blocks
    bad[first_pb], bad[0:8] = EMPTY << 30, [bad[first_pb]] + [EMPTY << 30] * 7
    assert T.builder_check(bad, T.plain_period, 0) != 0
    assert b"call schedule" in capi.lib().tetsim_last_error(None)
    bad = plain.copy()
    bad[0], bad[1] = plain[1], plain[0]                              # two tiles on each other's XCD
    assert T.builder_check(bad, T.plain_period, 0) != 0
    bad = plain.copy()
    bad[first_pb + 1] = bad[first_pb]                                # one particle block twice, one never
    assert T.builder_check(bad, T.plain_period, 0) != 0
    if tail:
        assert T.builder_check(entry, period, tail - 1) != 0
    wrapped_plain = plain.copy()                                     # a wrapped particle block that a tile at the head needs
    wrapped_plain[first_pb] |= 1 << 29
    assert T.builder_check(wrapped_plain, T.plain_period, T.plain_period) != 0
