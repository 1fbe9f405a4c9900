"""GPU: the march arithmetic of csrc/ngp_march.h where its shortened forms could part from the reference's: the scalings by the grid size H as one multiply
(`ngp_cell_coord`, `ngp_step_cells`, `ngp_face_plane`; the frame kernel's view only, whose H is a power of two), the exit face as an integer sum
(`ngp_exit_face`, every view) and the cascade picked by an integer clamp (`rv_consts::mip`).

Frames of 32 x 32 through `ngp_render_frame` (tests/_util.py render_frame) against the CPU oracle's cell-by-cell march
(oracle.render_oracle.render_single_march), compared as tests/test_gpu_frame_inside.py compares its constant-density frames (`_against_oracle` with a sample bar
of 0: the frame's sample total and its rays with samples are the oracle's exactly, image, weights_sum and depth inside that file's bars, equal depth masks), and
the same frame with block skipping and the occupied box switched off, one at a time and together, == bit for bit with the default route (`_differences`).

  cameras    `face0`: the eye on a cell face of cascade 0 on all three axes, min_near 0, so the first lattice point IS a face (cell coordinate a whole number,
             exit at the point itself); `face1`: the same on cascade 1's lattice, outside cascade 0 (two cascades), or on the last cell layer under the box's
             wall (one cascade); `axis`: 1,024 rays along +-x, +-y, +-z whose two small direction components are +-1e-4 * 2^[0, 6): 1 / d up to 1e4, no
             component 0 (those are tests/test_gpu_frame_inside.py's 33 x 33 frames)
  grids      one cascade at bound 1 and two at bound 2; H 64 and 128; random spheres (tests/_util.py blob_bitfield), few enough for long empty stretches
  steps      dt_gamma 0 (constant step: closed-form skips) and 1 / 128 (walked skips)

`test_per_op_march_on_the_same_rays`: `raymarching.march_rays` on the same rays against the oracle's `march_rays`, == on the bits of positions, directions and
both deltas: the per-op view (`ngp_march_t`) keeps the reference's sequence for the scalings by H and takes only the integer exit face.  A grid size that is not
a power of two cannot be marched by either route (H = 48 is refused by `march_rays` too: test_gpu_frame_inside.py
test_a_grid_size_that_is_not_a_power_of_two_is_refused), so this runs at H 64 and 128 like the frames."""
import numpy as np
import pytest
import torch

from _frame_poses import DENSITY, constant_field
from _util import blob_bitfield
from oracle import render_oracle as R
from test_gpu_frame_inside import _against_oracle, _differences, _frame

pytestmark = pytest.mark.gpu
F32 = np.float32
RES = 32
GRIDS = ((1.0, 1, 64), (1.0, 1, 128), (2.0, 2, 64), (2.0, 2, 128))               # bound, cascades, H


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cameras(bound, cascade):
    """name -> (rays_o, rays_d) float32 [RES * RES, 3].  2 / 64 and 4 / 64 divide every coordinate of the face eyes: they lie on cell faces at H 64 and at H 128."""
    from ngp import workload as W
    eyes = {"face0": ((0.25, -0.125, 0.0625), (0.6, -1.0, 0.35))}
    eyes["face1"] = ((1.5, 0.25, -1.25), (-1.0, -0.3, 0.7)) if cascade == 2 else ((-0.75, 0.5, 0.96875), (0.8, -0.5, -1.0))
    out = {name: W.get_rays(W.look_pose(eye, fwd), W.intrinsics(RES, RES), RES, RES) for name, (eye, fwd) in eyes.items()}
    rng = np.random.default_rng(21)
    n = RES * RES
    axis, sign = np.arange(n) % 3, np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
    d = np.zeros((n, 3))
    small = 1.0001e-4 * np.exp2(rng.uniform(0, 6, size=(n, 2))) * rng.choice([-1.0, 1.0], size=(n, 2))
    for k in range(3):
        rows = axis == k
        d[rows, k] = sign[rows]
        d[np.ix_(rows, [(k + 1) % 3, (k + 2) % 3])] = small[rows]
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    assert float(np.abs(d).min()) >= 1e-4 and float(np.abs(d).min()) < 2e-4
    o = np.broadcast_to(np.array([0.31, -0.17, 0.23], F32) * F32(bound), d.shape).copy()
    out["axis"] = (o, d)
    for name, (o, d) in out.items():
        assert o.dtype == F32 and d.dtype == F32 and not (d == 0).any(), name
    return out


@pytest.fixture(scope="module")
def grids(oracle, dev):
    """(bound, cascade, H) -> (bitfield, constant-density renderer over it): all-zero networks, sigma = DENSITY everywhere, so no ray saturates and every
    marched sample is composited (tests/test_gpu_frame_inside.py `constant`)"""
    from ngp.field import NGPFieldFF
    from ngp.render import NGPRenderer
    made = {}

    def get(bound, cascade, grid_h):
        key = (bound, cascade, grid_h)
        if key not in made:
            field = NGPFieldFF(bound=bound, density_scale=DENSITY).to(dev)
            with torch.no_grad():
                field.sigma_net.weights.zero_()
                field.color_net.weights.zero_()
            ren = NGPRenderer(field, bound=bound, cuda_ray=True, density_scale=DENSITY, density_thresh=0.5, grid_size=grid_h).to(dev).eval()
            bitfield, grid = blob_bitfield(oracle, cascade, grid_h, seed=7, n_blobs=40 if cascade == 1 else 14, bound=bound)   # every camera sees spheres
            ren.load_density_grid(grid)
            assert ren.cascade == cascade and np.array_equal(ren.density_bitfield.cpu().numpy(), bitfield) and 0 < int(grid.sum()) < grid.size
            made[key] = (bitfield, ren)
        return made[key]
    return get


@pytest.mark.parametrize("dt_gamma", (0.0, 1.0 / 128))
@pytest.mark.parametrize("bound,cascade,grid_h", GRIDS)
def test_frames_on_cell_faces_and_along_the_axes(oracle, dev, grids, bound, cascade, grid_h, dt_gamma):
    bitfield, ren = grids(bound, cascade, grid_h)
    failures = []
    for name, (o, d) in _cameras(bound, cascade).items():
        what = f"{name} bound {bound} C {cascade} H {grid_h} dt_gamma {dt_gamma:.4f}"
        ref = R.render_single_march(constant_field, o, d, bitfield, bound, cascade, H=grid_h, min_near=0.0, dt_gamma=dt_gamma)
        assert np.array_equal(ref["consumed"], ref["marched"]), what            # no ray saturates: every marched sample counts
        to, td = t(o, dev), t(d, dev)
        base, _ = _frame(ren, to, td, RES, dev, dt_gamma=dt_gamma, min_near=0.0)
        stats = _against_oracle(base, ref, what, sample_bar=0)
        assert int(stats[0]) == ref["samples"], (what, stats, ref["samples"])
        assert ref["samples"] > 1000, (what, ref["samples"])                    # the camera does see the spheres
        for route, kw in (("block skipping off", dict(block_skip=0)), ("occupied box off", dict(occupied_box=0)),
                          ("both off", dict(block_skip=0, occupied_box=0))):
            out, _ = _frame(ren, to, td, RES, dev, dt_gamma=dt_gamma, min_near=0.0, **kw)
            failures += [f"{what}, {route}: {line}" for line in _differences(out, base)]
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dt_gamma", (0.0, 1.0 / 128))
@pytest.mark.parametrize("bound,cascade,grid_h", GRIDS)
def test_per_op_march_on_the_same_rays(oracle, dev, grids, bound, cascade, grid_h, dt_gamma):
    import raymarching
    bitfield, _ = grids(bound, cascade, grid_h)
    cams = _cameras(bound, cascade)
    o = np.concatenate([cams[name][0] for name in cams])
    d = np.concatenate([cams[name][1] for name in cams])
    aabb = np.array([-bound] * 3 + [bound] * 3, F32)
    nears, fars = oracle.near_far_from_aabb(o, d, aabb, 0.0)
    n, n_step = o.shape[0], 128
    alive = np.arange(n, dtype=np.int32)
    x_ref, d_ref, l_ref = oracle.march_rays(n, n_step, alive, nears.copy(), o, d, bound, bitfield, cascade, grid_h, nears, fars, 128, False, dt_gamma, 1024)
    x, dd, l = raymarching.march_rays(n, n_step, t(alive, dev), t(nears.copy(), dev), t(o, dev), t(d, dev), bound, t(bitfield, dev), cascade, grid_h,
                                      t(nears, dev), t(fars, dev), 128, False, dt_gamma, 1024)
    per_ray = (l_ref[: n * n_step, 0] > 0).reshape(n, n_step).sum(1)
    assert int(per_ray.sum()) > 5000 and bool((per_ray == 0).any())
    for got, want, what in ((l, l_ref, "deltas"), (x, x_ref, "xyzs"), (dd, d_ref, "dirs")):
        got = got.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), \
            f"{what}: {int((got != want).sum())} values differ (bound {bound}, H {grid_h}, dt_gamma {dt_gamma})"
