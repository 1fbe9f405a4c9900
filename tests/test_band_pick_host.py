"""CPU: which band queue a wave of the frame kernel draws its next tile from (csrc/ngp_band_pick.h), through the host export that evaluates the
function the kernel calls (ngp_render_band_pick_host), and the switches around it (ngp_render_set_band_merge, ngp_render_set_band_hysteresis)."""
import ctypes

import numpy as np
import pytest

BANDS = 32


def _lib():
    import ngp_hip
    return ngp_hip, ngp_hip.lib()


def _ranges(n_rays):
    t = (n_rays + 63) // 64
    return [(64 * (t * b // BANDS), min(64 * (t * (b + 1) // BANDS), n_rays)) for b in range(BANDS)]


def _pick(heads, n_rays, xcd, *, perm=None, cost=None, dry=0, last=-1, h=1.0):
    """(band or -1, dry mask after the look)"""
    ngp_hip, L = _lib()
    heads = np.ascontiguousarray(heads, np.uint32)
    assert heads.shape == (BANDS,)
    keep = [heads]
    p = c = None
    if perm is not None:
        perm, cost = np.ascontiguousarray(perm, np.uint32), np.ascontiguousarray(cost, np.uint32)
        keep += [perm, cost]
        p, c = perm.ctypes.data, cost.ctypes.data
    band, mask = ctypes.c_int(-7), ctypes.c_uint32(0)
    rc = L.raw.ngp_render_band_pick_host(heads.ctypes.data, n_rays, p, c, xcd, dry, last, h, ctypes.addressof(band), ctypes.addressof(mask))
    ngp_hip.check(rc, "band_pick_host")
    return band.value, mask.value


def _rank(b, x):
    return (((b & 7) - x) & 7) * 4 + (b >> 3)


def _frame(n_tiles, costs_by_band=None, seed=0):
    """a frame of n_tiles tiles: identity order within each band, cost[tile] decreasing within each band (as k_tile_sort leaves it)"""
    n_rays = 64 * n_tiles
    perm = np.arange(n_tiles, dtype=np.uint32)
    cost = np.zeros(n_tiles, np.uint32)
    rng = np.random.default_rng(seed)
    for b, (lo, hi) in enumerate(_ranges(n_rays)):
        n = (hi - lo) // 64
        c = np.sort(rng.integers(1, 5000, size=n))[::-1] if costs_by_band is None else np.asarray(costs_by_band[b][:n])
        cost[lo // 64:hi // 64] = c
    return n_rays, perm, cost


def test_switches_are_exported_and_return_the_previous_value():
    import os
    ngp_hip, L = _lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngp_hip.h")).read()
    for name in ("ngp_render_set_band_merge", "ngp_render_set_band_hysteresis", "ngp_render_band_pick_host"):
        assert name in ngp_hip.EXPORTS and name + "(" in header
    # the issue asked for "on by default" if the A/B against the parent showed a gain, and for "off" otherwise: the merge's own gain stayed inside the
    # run-to-run spread (profiles/HISTORY.md 5.8), so it is off
    assert L.ngp_render_set_band_merge(1) == 0                   # default off
    try:
        assert L.ngp_render_set_band_merge(0) == 1
        assert L.ngp_render_set_band_merge(7) == 0               # any non-zero value means on
        assert L.ngp_render_set_band_merge(0) == 1
    finally:
        L.ngp_render_set_band_merge(0)
    default_h = L.ngp_render_set_band_hysteresis(2.0)
    try:
        assert default_h == 4.0
        assert L.ngp_render_set_band_hysteresis(0.25) == 2.0     # below 1 means 1
        assert L.ngp_render_set_band_hysteresis(1000.0) == 1.0   # above 64 means 64
        assert L.ngp_render_set_band_hysteresis(1.5) == 64.0
        assert L.ngp_render_set_band_hysteresis(default_h) == 1.5
    finally:
        L.ngp_render_set_band_hysteresis(default_h)


@pytest.mark.parametrize("x", range(8))
def test_own_bands_come_before_foreign_ones_and_the_larger_estimate_wins(x):
    n_rays, perm, cost = _frame(32 * 6, seed=x)
    heads = np.zeros(BANDS, np.uint32)
    ranges = _ranges(n_rays)
    # make a foreign band's next tile the most expensive of the frame: an own band is picked all the same
    foreign = (x + 3) & 7
    cost[ranges[foreign][0] // 64] = 1_000_000
    own = [x, x + 8, x + 16, x + 24]
    band, _ = _pick(heads, n_rays, x, perm=perm, cost=cost)
    nxt = {b: int(cost[perm[ranges[b][0] // 64]]) for b in own}
    best = max(nxt.values())
    assert band in own and nxt[band] == best
    assert band == min((b for b in own if nxt[b] == best), key=lambda b: _rank(b, x))
    # heads move the look: after 3 tiles of `band` its next estimate is the fourth's
    heads[band] = 3 * 64
    nxt[band] = int(cost[perm[ranges[band][0] // 64 + 3]])
    band2, _ = _pick(heads, n_rays, x, perm=perm, cost=cost)
    assert nxt[band2] == max(nxt.values())
    # with the own bands dry the foreign band with the most expensive next tile is next
    band3, mask = _pick(heads, n_rays, x, perm=perm, cost=cost, dry=sum(1 << b for b in own))
    assert band3 == foreign and mask == sum(1 << b for b in own)


def test_ties_go_to_the_lower_rank():
    n_rays, perm, cost = _frame(32 * 4, costs_by_band=[[70, 50, 30, 10]] * BANDS)
    for x in range(8):
        heads = np.zeros(BANDS, np.uint32)
        assert _pick(heads, n_rays, x, perm=perm, cost=cost)[0] == x
        heads[x] = 64                                             # x's next is 50 now: x + 8 (70) leads, then x + 16, x + 24
        assert _pick(heads, n_rays, x, perm=perm, cost=cost)[0] == x + 8
        heads[x + 8] = 64
        assert _pick(heads, n_rays, x, perm=perm, cost=cost)[0] == x + 16
        heads[x + 16] = heads[x + 24] = 64                        # all four at 50 again
        assert _pick(heads, n_rays, x, perm=perm, cost=cost)[0] == x


@pytest.mark.parametrize("n_rays", [64, 128, 64 * 45, 64 * 625, 200 * 204, 70])
def test_a_dry_or_empty_band_is_never_returned_and_all_dry_returns_none(n_rays):
    """walk a frame to its end from every XCD, with random estimates where the frame has whole tiles: every pick has rays left, no empty band's
    perm / cost is read (they are exactly n_tiles long: numpy arrays, a read past them would at best return garbage, which the asserts below catch
    as a pick of a band without rays), and the walk ends with 'none' and a full mask"""
    ranges = _ranges(n_rays)
    n_tiles = (n_rays + 63) // 64
    rng = np.random.default_rng(n_rays)
    perm = cost = None
    if n_rays % 64 == 0:
        perm = np.arange(n_tiles, dtype=np.uint32)
        cost = rng.integers(0, 1000, size=n_tiles).astype(np.uint32)
    for x in range(8):
        heads, dry, last, drawn = np.zeros(BANDS, np.uint32), 0, -1, 0
        for _ in range(n_tiles + 2 * BANDS + 1):
            band, dry = _pick(heads, n_rays, x, perm=perm, cost=cost, dry=dry, last=last)
            if band < 0:
                break
            lo, hi = ranges[band]
            assert not (dry >> band) & 1 and lo + heads[band] < hi, (band, lo, hi, heads[band])
            drawn += min(64, hi - lo - int(heads[band]))
            heads[band] += 64                                     # the kernel's atomicAdd
            if lo + heads[band] >= hi:
                dry |= 1 << band
            last = band
        assert band == -1 and dry == 0xFFFFFFFF and drawn == n_rays
        assert _pick(heads, n_rays, x, perm=perm, cost=cost, dry=0)[0] == -1        # the heads alone say so, too


@pytest.mark.parametrize("x", range(8))
@pytest.mark.parametrize("estimates", ["none", "all equal"])
def test_with_equal_estimates_the_bands_are_walked_in_the_static_order(x, estimates):
    n_rays = 64 * 32 * 3
    perm = cost = None
    if estimates == "all equal":
        perm, cost = np.arange(32 * 3, dtype=np.uint32), np.full(32 * 3, 17, np.uint32)
    expected = [((x + k) & 7) + 8 * j for k in range(8) for j in range(4)]
    heads, dry, last, walked = np.zeros(BANDS, np.uint32), 0, -1, []
    ranges = _ranges(n_rays)
    for h in (1.0, 2.0):
        heads[:], dry, last, walked = 0, 0, -1, []
        while True:
            band, dry = _pick(heads, n_rays, x, perm=perm, cost=cost, dry=dry, last=last, h=h)
            if band < 0:
                break
            if not walked or walked[-1] != band:
                walked.append(band)
            heads[band] += 64
            if ranges[band][0] + heads[band] >= ranges[band][1]:
                dry |= 1 << band
            last = band
        assert walked == expected


def test_hysteresis_keeps_the_wave_on_its_band_until_another_exceeds_h_times():
    x = 2
    by_band = [[100, 100, 100]] * BANDS
    n_rays, perm, cost = _frame(32 * 3, costs_by_band=by_band)
    ranges = _ranges(n_rays)
    heads = np.zeros(BANDS, np.uint32)

    def set_next(b, value):
        cost[perm[(ranges[b][0] + int(heads[b])) // 64]] = value
    set_next(x + 8, 199)
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x, h=1.0)[0] == x + 8        # pure merge: the larger estimate
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x, h=2.0)[0] == x            # 199 does not exceed 2 x 100
    set_next(x + 8, 200)
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x, h=2.0)[0] == x            # nor does 200: only MORE than h times
    set_next(x + 8, 201)
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x, h=2.0)[0] == x + 8
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x, h=4.0)[0] == x
    set_next(x + 8, 401)
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x, h=4.0)[0] == x + 8
    # an equal estimate elsewhere never pulls the wave off its band, whatever its rank; without a last band the lower rank wins
    set_next(x + 8, 100)
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x + 16, h=1.0)[0] == x + 16
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=-1, h=1.0)[0] == x
    # the last band counts only while it has tiles, and only when it is one of the XCD's own
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x + 16, dry=1 << (x + 16), h=4.0)[0] == x
    set_next(x + 8, 150)
    assert _pick(heads, n_rays, x, perm=perm, cost=cost, last=x + 1, h=4.0)[0] == x + 8


def test_bad_arguments_are_refused():
    _, L = _lib()
    heads = np.zeros(BANDS, np.uint32)
    band = ctypes.c_int(0)
    args = lambda **kw: [kw.get("heads", heads.ctypes.data), 640, None, None, kw.get("xcd", 0), 0, kw.get("last", -1), 1.0,   # noqa: E731
                         kw.get("out", ctypes.addressof(band)), None]
    assert L.raw.ngp_render_band_pick_host(*args()) == 0
    for bad in (dict(heads=None), dict(xcd=8), dict(last=32), dict(last=-2), dict(out=None)):
        assert L.raw.ngp_render_band_pick_host(*args(**bad)) != 0
