"""GPU: a wave of the frame kernel picks the band it draws its next tile from by the estimate of that tile (csrc/ngp_band_pick.h, render_fused.hip's
refill; ngp_render_set_band_merge, ngp_render_set_band_hysteresis).  The pick changes when a tile is rendered, never what it computes: with the merge on,
with it off and with the tile order off, images, depths, weights and statistics are bit-identical and every pixel is written.  The frames are the
smallest that can break the pick: one tile (31 empty bands), two, fewer tiles than waves, and frames without a tile order."""
import contextlib

import numpy as np
import pytest
import torch

from _util import render_frame  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(dev):
    from ngp import workload as W
    from ngp.field import NGPFieldFF
    from ngp.render import NGPRenderer
    field = NGPFieldFF(bound=W.BOUND).to(dev).load_arrays(W.make_model(0))

    def renderer(grid):
        ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
        ren.load_density_grid(grid)
        return ren
    grid = W.density_grid()
    return dict(W=W, ring=renderer(grid), full=renderer(np.full_like(grid, 100.0)), empty=renderer(np.zeros_like(grid)))


@contextlib.contextmanager
def band_merge(enabled, h=None):
    """the process-wide switch and the hysteresis for the block, restored afterwards"""
    import ngp_hip
    L = ngp_hip.lib()
    before = L.ngp_render_set_band_merge(int(enabled))
    before_h = L.ngp_render_set_band_hysteresis(float(h)) if h is not None else None
    try:
        yield
    finally:
        L.ngp_render_set_band_merge(before)
        if before_h is not None:
            L.ngp_render_set_band_hysteresis(before_h)


def default_h():
    import ngp_hip
    L = ngp_hip.lib()
    h = L.ngp_render_set_band_hysteresis(1.0)
    L.ngp_render_set_band_hysteresis(h)
    return h


def _render(ren, o, d, width, *, merge, order=1, h=None):
    import ngp_hip
    with band_merge(merge, h):
        out, _, rc = render_frame(ren, o, d, width, tile_order=order)
    ngp_hip.check(rc, "render_frame")
    return out


def _same(a, b, what):
    for key in ("image", "depth", "weights_sum"):
        assert not bool(torch.isnan(a[key]).any()) and not bool(torch.isnan(b[key]).any()), f"{what}: {key}: a pixel was not written"
        assert torch.equal(a[key], b[key]), f"{what}: {key}: {int((a[key] != b[key]).sum())} values differ"
    assert torch.equal(a["stats"][:3], b["stats"][:3]), f"{what}: stats {a['stats'].tolist()} {b['stats'].tolist()}"


def _check(ren, W, pose, width, height, dev, hint=None):
    o, d = W.get_rays(pose, W.intrinsics(height, width), height, width)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    hint = width if hint is None else hint
    off = _render(ren, o, d, hint, merge=0)
    plain = _render(ren, o, d, hint, merge=0, order=0)
    _same(off, plain, "merge off | tile order off")
    for h in (1.0, default_h()):
        on = _render(ren, o, d, hint, merge=1, h=h)
        _same(on, off, f"merge on (h = {h}) | merge off")
        _same(on, plain, f"merge on (h = {h}) | tile order off")
    return off


# width x height; (200, 204) is 204 pixels wide: no 8x8 tiles, so no tile order, and the static sequence runs
@pytest.mark.parametrize("width,height,hint", [(8, 8, None), (8, 16, None), (72, 40, None), (64, 64, None), (200, 200, None), (204, 200, None), (200, 200, 0)])
def test_small_frames(scene, dev, width, height, hint):
    W = scene["W"]
    out = _check(scene["ring"], W, W.orbit_pose(2), width, height, dev, hint)
    if width * height >= 64 * 64:
        assert int(out["stats"][0]) > 0


@pytest.mark.parametrize("height", [-1.2, 1.5])
def test_below_and_above_the_scene(scene, dev, height):
    W = scene["W"]
    out = _check(scene["ring"], W, W.orbit_pose(1, height=height), 200, 200, dev)
    assert int(out["stats"][0]) > 0


def test_from_inside_the_scene(scene, dev):
    import _frame_poses as FP
    out = _check(scene["ring"], scene["W"], FP.pose("centre"), 200, 200, dev)
    assert int(out["stats"][0]) > 0


def test_full_grid_where_every_estimate_ties(scene, dev):
    W = scene["W"]
    out = _check(scene["full"], W, W.orbit_pose(3), 200, 200, dev)
    assert int(out["stats"][0]) > 0


def test_empty_grid_where_every_estimate_is_zero(scene, dev):
    W = scene["W"]
    out = _check(scene["empty"], W, W.orbit_pose(3), 200, 200, dev)
    assert int(out["stats"][0]) == 0 and int(out["stats"][2]) == 0              # every ray misses


def test_two_poses_in_one_launch(scene, dev):
    """ngp_render_frames_camera keeps its row-major tiles and the static band sequence: equal with the switch on and off"""
    W, ren = scene["W"], scene["ring"]
    poses = np.stack([W.orbit_pose(k) for k in (1, 5)]).astype(np.float32)
    intr = W.intrinsics(64, 64)
    outs = {}
    for mode in (1, 0):
        with band_merge(mode):
            outs[mode] = ren.render_fused_cameras(poses, intr, 64, 64, bg_color=1)
            torch.cuda.synchronize()
    for key in ("image", "depth", "weights_sum"):
        assert not bool(torch.isnan(outs[1][key]).any()), key
        assert torch.equal(outs[0][key], outs[1][key]), key
    assert torch.equal(outs[0]["stats"][:3], outs[1]["stats"][:3])
    with band_merge(1):
        one = ren.render_fused_camera(poses[1], intr, 64, 64, bg_color=1)
        torch.cuda.synchronize()
    assert torch.equal(one["image"].reshape(-1), outs[1]["image"][1].reshape(-1))
