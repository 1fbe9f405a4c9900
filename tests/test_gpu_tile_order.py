"""GPU: the frame kernel hands out each band's 8x8 tiles by decreasing estimated cost and lets each XCD take its bands by decreasing total
(render_fused.hip: k_tile_cost, k_tile_sort).  The order changes when a ray is rendered, never what it computes: with the switch on and off,
images, depths, weights and statistics are bit-identical, every pixel is written, and the order read back from the workspace is a permutation
of each band's tiles."""
import numpy as np
import pytest
import torch

from _util import FRAME_WS_AREA as WS_AREA, render_frame  # noqa: E402

pytestmark = pytest.mark.gpu

BANDS = 32


@pytest.fixture(scope="module")
def scene(dev):
    from ngp import workload as W
    from ngp.field import NGPFieldFF
    from ngp.render import NGPRenderer
    model = W.make_model(0)
    field = NGPFieldFF(bound=W.BOUND).to(dev).load_arrays(model)

    def renderer(grid):
        ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
        ren.load_density_grid(grid)
        return ren
    grid = W.density_grid()
    return dict(W=W, ren=renderer(grid), full=renderer(np.full_like(grid, 100.0)))


def _render(ren, o, d, width, order):
    """ngp_render_frame as NGPRenderer.render_fused calls it, with NaN-filled outputs; returns the outputs and the workspace."""
    import ngp_hip as H
    out, ws, rc = render_frame(ren, o, d, width, tile_order=order)
    H.check(rc, "render_frame")
    return out, ws


def _check(ren, W, pose, res, dev, width=None):
    o, d = W.get_rays(pose, W.intrinsics(res[0], res[1]), res[0], res[1])
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    width = res[1] if width is None else width
    a, ws = _render(ren, o, d, width, 1)
    b, _ = _render(ren, o, d, width, 0)
    for key in ("image", "depth", "weights_sum"):
        assert not bool(torch.isnan(a[key]).any()), f"{key}: a pixel was not written"
        assert torch.equal(a[key], b[key]), f"{key}: {int((a[key] != b[key]).sum())} values differ"
    assert torch.equal(a["stats"][:3], b["stats"][:3])
    return a, ws


def _perm_per_band(ws, n_tiles):
    perm = ws[WS_AREA:WS_AREA + 4 * n_tiles].view(torch.int32).cpu().numpy().astype(np.int64)
    cost = ws[WS_AREA + 4 * n_tiles:WS_AREA + 8 * n_tiles].view(torch.int32).cpu().numpy().astype(np.int64)
    for b in range(BANDS):
        lo, hi = n_tiles * b // BANDS, n_tiles * (b + 1) // BANDS
        p = perm[lo:hi]
        assert np.array_equal(np.sort(p), np.arange(lo, hi)), f"band {b}: not a permutation of its tiles"
        c = cost[p]
        assert bool((c[:-1] >= c[1:]).all()), f"band {b}: tiles not in decreasing cost"
    return perm, cost


@pytest.mark.parametrize("k", range(8))
def test_orbit_poses(scene, dev, k):
    W = scene["W"]
    out, ws = _check(scene["ren"], W, W.orbit_pose(k), (800, 800), dev)
    assert int(out["stats"][0]) > 10_000_000
    _, cost = _perm_per_band(ws, 800 * 800 // 64)
    assert cost.max() > 0


@pytest.mark.parametrize("height", [-1.2, 1.5])
def test_below_and_above_the_scene(scene, dev, height):
    W = scene["W"]
    out, ws = _check(scene["ren"], W, W.orbit_pose(1, height=height), (800, 800), dev)
    assert int(out["stats"][0]) > 0
    _perm_per_band(ws, 800 * 800 // 64)


def test_full_grid(scene, dev):
    W = scene["W"]
    out, ws = _check(scene["full"], W, W.orbit_pose(3), (800, 800), dev)
    _perm_per_band(ws, 800 * 800 // 64)


def test_small_frame_and_a_width_that_is_not_a_multiple_of_eight(scene, dev):
    W = scene["W"]
    _, ws = _check(scene["ren"], W, W.orbit_pose(2), (200, 200), dev)
    _perm_per_band(ws, 200 * 200 // 64)
    _check(scene["ren"], W, W.orbit_pose(2), (200, 204), dev)    # tile_w = 0: rays in plain order, no tile order
    _check(scene["ren"], W, W.orbit_pose(2), (200, 200), dev, width=0)


def test_several_frames_per_launch(scene, dev):
    """ngp_render_frames_camera (8 poses, one launch) keeps its row-major tiles (the drain is shared by the frames): bit-equal with the switch on
    and off, and equal to one launch per pose, which is ordered."""
    import ngp_hip as H
    W, ren = scene["W"], scene["ren"]
    poses = np.stack([W.orbit_pose(k) for k in range(8)]).astype(np.float32)
    intr = W.intrinsics(800, 800)
    L = H.lib()
    outs = {}
    for mode in (1, 0):
        previous = L.ngp_render_set_tile_order(mode)
        try:
            outs[mode] = ren.render_fused_cameras(poses, intr, 800, 800, bg_color=1, return_workspace=True)
            torch.cuda.synchronize()
        finally:
            L.ngp_render_set_tile_order(previous)
    for key in ("image", "depth", "weights_sum"):
        assert torch.equal(outs[0][key], outs[1][key]), key
    assert torch.equal(outs[0]["stats"][:3], outs[1]["stats"][:3])

    one = ren.render_fused_camera(poses[5], intr, 800, 800, bg_color=1)
    assert torch.equal(one["image"].reshape(-1), outs[1]["image"][5].reshape(-1))
