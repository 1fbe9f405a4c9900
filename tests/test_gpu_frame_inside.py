"""GPU: the frame kernel (render_fused.hip: ngp_render_frame) with the camera INSIDE the scene, and every route its launcher can take.

Every other frame test looks at the scene from an orbit outside everything occupied.  The poses of tests/_frame_poses.py put the eye among the pillars, in
a pillar, in the ground slab, under a lintel, just inside the AABB's wall, and outside the occupied box looking away: the second slab test of the refill
with the origin inside the box of everything occupied and with the box behind the camera, a march that starts in the middle of an occupied 4^3 / 16^3 block,
level axis-aligned poses whose centre column and row have direction components of exactly 0.0 (33 x 33; 40 x 40 is the size that qualifies for 8x8 tiles),
min_near 0.2, 0.05 and 0, frames without a single sample.  The checker is the CPU oracle's cell-by-cell march (oracle.render_oracle.render_single_march).

  part 2  test_constant_density_sample_counts: a constant small density, so that no ray saturates and every marched sample is composited: the totals are
          EXACTLY the oracle's, and with a constant step every ray's weights_sum is a strictly increasing function of its own sample count
  part 3  test_real_field_from_inside: the make_model field, the bars of test_gpu_fused_variants.check plus test_gpu_church's depth bar
  part 4  test_every_route_gives_the_same_frame, test_cameras_give_the_frame_of_rays_in_memory: bit-identity with the default route
          test_small_grids_against_the_oracle, test_three_cascades_that_are_not_nested: routes that differ by the grid, against the oracle

The launcher's routes (rv_render_frame) and the test that pins each for ngp_render_frame:

  route                                                condition                                           test
  map, skipping, box, tile order                       2 cascades, bound a power of two, H 128              parts 2, 3 at bound 2.0; the default of part 4
  map, no skipping, no box                             2 cascades, bound 1.5                                parts 2, 3 at bound 1.5
  one cascade, box lattice not dyadic                  bound 0.75: occ_unit = 2 * 0.75 / 32                 part 2 at bound 0.75
  map, each switch off                                 ngp_render_set_occupied_box / _block_skip / _tile_order   test_every_route_gives_the_same_frame
  no map: bitfield not 8-byte aligned                  (bitfield & 7) != 0                                  test_every_route_gives_the_same_frame
  no map: workspace of the header only                 workspace_bytes = 256 (below: refused)               test_every_route_gives_the_same_frame
  map, no tile order: no permutation area              workspace_bytes = 256 + 48 KiB                       test_every_route_gives_the_same_frame
  no tiles                                             image_width 0; 33 x 33                               test_every_route_gives_the_same_frame, parts 2, 3
  camera in the kernel, several frames a launch        ngp_render_frame_camera, ngp_render_frames_camera    test_cameras_give_the_frame_of_rays_in_memory
  no map: H 4, 8; map without skipping or box: H 16    blocks_per_level % 32 != 0; H < 64                   test_small_grids_against_the_oracle
  no map: 3 cascades, not nested                       bound 3.0 (LDS carve)                                test_three_cascades_that_are_not_nested
  refused: a grid size that is not a power of two      Morton index beyond H^3                              test_a_grid_size_that_is_not_a_power_of_two_is_refused
"""
import numpy as np
import pytest
import torch

import _frame_poses as FP
from _frame_checks import _same_count_same_weight, _written
from _util import FRAME_WS_AREA, FRAME_WS_HEADER, blob_bitfield, render_frame
from oracle import render_oracle as R

pytestmark = pytest.mark.gpu

ODD, EVEN = 33, 40                  # exact-zero direction components | a multiple of 8: the rays are handed out in 8x8 tiles
BOUNDS = (2.0, 1.5, 0.75)           # 2 nested cascades | 2 cascades that are not nested (no skipping, no box) | 1 cascade, box lattice 0.046875


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def constant(dev):
    """bound -> renderer of the ring scene's grid over all-zero networks (test_gpu_fullsize._constant_density_renderer at any bound): sigma = FP.DENSITY
    everywhere, so no ray saturates and a ray's weights_sum is a strictly increasing function of its sample count"""
    from ngp import workload as W
    from ngp.field import NGPFieldFF
    from ngp.render import NGPRenderer
    made = {}

    def get(bound):
        if bound not in made:
            field = NGPFieldFF(bound=bound, density_scale=FP.DENSITY).to(dev)
            with torch.no_grad():
                field.sigma_net.weights.zero_()
                field.color_net.weights.zero_()
            ren = NGPRenderer(field, bound=bound, cuda_ray=True, density_scale=FP.DENSITY, density_thresh=10.0).to(dev).eval()
            ren.load_density_grid(W.density_grid(bound=bound))
            bitfield, cascade = FP.scene(bound)
            assert ren.cascade == cascade and np.array_equal(ren.density_bitfield.cpu().numpy(), bitfield)
            made[bound] = ren
        return made[bound]
    return get


@pytest.fixture(scope="module")
def real(dev):
    """bound -> (model, renderer) of workload.make_model(0, bound) on the ring scene's grid, as test_gpu_fused_variants.build"""
    from ngp import workload as W
    from ngp.field import NGPFieldFF
    from ngp.render import NGPRenderer
    made = {}

    def get(bound):
        if bound not in made:
            model = W.make_model(0, bound=bound)
            field = NGPFieldFF(bound=bound).to(dev).load_arrays(model)
            ren = NGPRenderer(field, bound=bound, cuda_ray=True, density_thresh=10.0).to(dev).eval()
            ren.load_density_grid(W.density_grid(bound=bound))
            assert np.array_equal(ren.density_bitfield.cpu().numpy(), FP.scene(bound)[0])
            made[bound] = (model, ren)
        return made[bound]
    return get


def _frame(ren, o, d, width, dev, **kw):
    import ngp_hip
    out, ws, rc = render_frame(ren, t(o, dev) if isinstance(o, np.ndarray) else o, t(d, dev) if isinstance(d, np.ndarray) else d, width, **kw)
    ngp_hip.check(rc, "render_frame")
    return out, ws


def _against_oracle(out, ref, what, sample_bar):
    """the bars of test_gpu_fused_variants.check (image and weights_sum 5e-3, rays with samples exact, the sample total within `sample_bar`) and of
    test_gpu_church (depth 2e-3 on the reference's finite pixels, equal finiteness masks); the figures are printed before anything is asserted"""
    stats = out["stats"].cpu().numpy()
    img, ws, dep = out["image"].cpu().numpy(), out["weights_sum"].cpu().numpy(), out["depth"].cpu().numpy()
    ok = np.isfinite(ref["depth"])
    same_mask = np.array_equal(np.isfinite(dep), ok)
    e_img, e_ws = float(np.max(np.abs(img - ref["image"]))), float(np.max(np.abs(ws - ref["weights_sum"])))
    e_dep = float(np.max(np.abs(dep[ok] - ref["depth"][ok]))) if same_mask and ok.any() else 0.0
    hit = int((ref["consumed"] > 0).sum())
    print(f"{what}: samples {int(stats[0])} (oracle {ref['samples']}, bar {sample_bar:g}), capped {int(stats[1])}, rays hit {int(stats[2])} (oracle {hit}), "
          f"image {e_img:.2e}, weights_sum {e_ws:.2e}, depth {e_dep:.2e}, depth masks equal {same_mask}")
    _written(out, what)
    assert abs(int(stats[0]) - ref["samples"]) <= sample_bar, (what, stats, ref["samples"])
    assert stats[2] == hit, (what, stats, hit)
    assert e_img < 5e-3 and e_ws < 5e-3, (what, e_img, e_ws)
    assert same_mask, f"{what}: depth is finite on {int(np.isfinite(dep).sum())} rays, the oracle's on {int(ok.sum())}"
    assert e_dep < 2e-3, (what, e_dep)
    return stats


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part 1: the pose table, on the reference
# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FP.NAMES)
def test_pose_table_on_the_reference(oracle, name):
    """what each pose is in the table for (tests/_frame_poses.py: check_reaches) holds at the two sizes rendered here; 66 direction components are exactly
    zero in the axis-aligned poses at 33 x 33, in_solid gives every ray samples at min_near 0 and fewer at 0.2, three poses give no sample at all"""
    for res in (ODD, EVEN):
        refs = {mn: FP.reference_constant(name, res, 2.0, min_near=mn) for mn in (0.2, 0.0)}
        FP.check_reaches(name, res, refs)
    assert FP.ZERO_COMPONENTS["centre"] * ODD == 66


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part 2: exact sample counts from inside
# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("min_near", (0.2, 0.05, 0.0))
@pytest.mark.parametrize("dt_gamma", (0.0, 1.0 / 128))
@pytest.mark.parametrize("name", FP.NAMES)
def test_constant_density_sample_counts(oracle, dev, constant, name, dt_gamma, min_near, bound):
    """Conditions, not tolerances: the frame's sample total, its capped rays (none) and its rays with samples are the oracle's exactly; with a constant
    step (dt_gamma 0) rays with equal counts in the oracle have bit-equal weights_sum, more samples strictly more, none exactly 0; depth is finite exactly
    where the oracle's is.  With dt_gamma > 0 the step differs from ray to ray, so the per-ray argument does not apply: the totals and the image bars do.
    The reference is first checked to be inside what makes this valid (FP.check_reference_is_clean)."""
    ren = constant(bound)
    for res in (ODD, EVEN):
        what = f"{name} {res}x{res} bound {bound} min_near {min_near} dt_gamma {dt_gamma:.4f}"
        o, d = FP.rays(name, res)
        ref = FP.reference_constant(name, res, bound, min_near=min_near, dt_gamma=dt_gamma)
        FP.check_reference_is_clean(ref, bound)
        out, _ = _frame(ren, o, d, res, dev, dt_gamma=dt_gamma, min_near=min_near)
        stats = _against_oracle(out, ref, what, sample_bar=0)
        assert int(stats[0]) == ref["samples"] and int(stats[1]) == 0 and int(stats[2]) == int((ref["consumed"] > 0).sum()), (what, stats)
        if dt_gamma == 0.0:
            _same_count_same_weight(out["weights_sum"].cpu().numpy(), ref["marched"], what)
        else:
            assert bool((out["weights_sum"].cpu().numpy()[ref["marched"] == 0] == 0).all()), what


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part 3: the real field from inside
# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", (2.0, 1.5))
@pytest.mark.parametrize("name", FP.NAMES)
def test_real_field_from_inside(oracle, dev, real, name, bound):
    """make_model's field (rays that saturate inside the solids, early termination) against the oracle's single march with R.field_forward"""
    model, ren = real(bound)
    bitfield, cascade = FP.scene(bound)
    for res in (ODD, EVEN):
        o, d = FP.rays(name, res)
        ref = R.render_single_march(lambda x, dd: R.field_forward(model, x, dd, 1.0), o, d, bitfield, bound, cascade)
        assert (ref["samples"] == 0) == (name in FP.NO_SAMPLES)
        out, _ = _frame(ren, o, d, res, dev)
        stats = _against_oracle(out, ref, f"{name} {res}x{res} bound {bound}", sample_bar=max(8, 3e-4 * ref["samples"]))
        assert int(stats[1]) == 0


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part 4: every route gives the same frame
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _route_rays(name, res):
    from ngp import workload as W
    if name == "orbit":
        return W.get_rays(W.orbit_pose(1), W.intrinsics(res, res), res, res)
    return FP.rays(name, res)


def _differences(a, b):
    """[] when two frames are bit-identical in image, depth (NaN = NaN), weights_sum and the three order-independent statistics"""
    bad = []
    for key in ("image", "depth", "weights_sum"):
        x, y = a[key].reshape(-1), b[key].reshape(-1)
        if key == "depth":
            x, y = x.nan_to_num(), y.nan_to_num()
        if not torch.equal(x, y):
            where = torch.nonzero(x != y).reshape(-1)
            bad.append(f"{key}: {where.numel()} values differ, first at {int(where[0])}: {float(x[where[0]])!r} against {float(y[where[0]])!r}")
    if not torch.equal(a["stats"][:3], b["stats"][:3]):
        bad.append(f"stats {a['stats'][:3].tolist()} against {b['stats'][:3].tolist()}")
    return bad


@pytest.mark.parametrize("name", ("centre", "in_solid", "away", "orbit"))
@pytest.mark.parametrize("kind", ("constant", "real"))
def test_every_route_gives_the_same_frame(dev, constant, real, kind, name):
    """The launcher's comments say that none of its routes changes a result ("results are identical either way"; each ray's arithmetic is its own): every
    route below gives, bit for bit, the frame of the default route, and writes every output element.  All differences are collected before the test fails."""
    import ngp_hip
    L = ngp_hip.lib()
    ren = constant(2.0) if kind == "constant" else real(2.0)[1]
    n_bits = ren.density_bitfield.numel()
    holder = torch.zeros(n_bits + 16, dtype=torch.uint8, device=dev)
    shifted = holder[4:4 + n_bits]
    shifted.copy_(ren.density_bitfield)
    assert ren.density_bitfield.data_ptr() % 8 == 0 and shifted.data_ptr() % 8 == 4 and torch.equal(shifted, ren.density_bitfield)
    failures = []
    for res in (EVEN, ODD):
        N = res * res
        assert L.ngp_render_frame_workspace(N) == FRAME_WS_AREA + 8 * ((N + 63) // 64) and FRAME_WS_HEADER == 256
        o, d = _route_rays(name, res)
        o, d = t(o, dev), t(d, dev)
        base, ws = _frame(ren, o, d, res, dev)
        _written(base, f"{name} {res} default")
        assert not bool(torch.isnan(base["depth"]).any())                  # every eye lies inside the AABB: every depth is a number
        assert not bool((ws[FRAME_WS_HEADER:FRAME_WS_HEADER + 8192] == 0xAB).all()), "the default route built no coarse map"
        tiled = res % 8 == 0
        assert bool((ws[FRAME_WS_AREA:] == 0xAB).all()) != tiled, "the default route orders the tiles exactly when the image qualifies for them"
        routes = {
            "occupied box off": dict(occupied_box=0),
            "block skipping off": dict(block_skip=0),
            "tile order off": dict(tile_order=0),
            "all three switches off": dict(occupied_box=0, block_skip=0, tile_order=0),
            "bitfield at a 4-byte offset": dict(bitfield=shifted),
            "workspace of the header only": dict(workspace_bytes=FRAME_WS_HEADER),
            "workspace without the permutation area": dict(workspace_bytes=FRAME_WS_AREA),
            "image_width 0": dict(width=0),
        }
        for route, kw in routes.items():
            kw = dict(kw)
            out, ws_r = _frame(ren, o, d, kw.pop("width", res), dev, **kw)
            for key in ("image", "depth", "weights_sum"):
                if bool(torch.isnan(out[key]).any()):
                    failures.append(f"{res}x{res} {route}: {key}: {int(torch.isnan(out[key]).sum())} values were not written")
            failures += [f"{res}x{res} {route}: {line}" for line in _differences(out, base)]
            if route == "bitfield at a 4-byte offset":
                assert bool((ws_r[FRAME_WS_HEADER:FRAME_WS_HEADER + 8192] == 0xAB).all()), "a map was built from a bitfield that is not 8-byte aligned"
            if route in ("tile order off", "image_width 0"):
                assert bool((ws_r[FRAME_WS_AREA:] == 0xAB).all()), f"{route}: a tile order was written"
        # the switches are back where they were
        for setter in (L.ngp_render_set_occupied_box, L.ngp_render_set_block_skip, L.ngp_render_set_tile_order):
            assert setter(1) == 1
        # below the header's size the call is refused with an error code and renders nothing
        out, _, rc = render_frame(ren, o, d, res, workspace_bytes=FRAME_WS_HEADER - 1)
        assert rc < 0 and bool(torch.isnan(out["image"]).all()) and bool(torch.isnan(out["weights_sum"]).all()), rc
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ("constant", "real"))
def test_cameras_give_the_frame_of_rays_in_memory(dev, constant, real, kind):
    """ngp_render_frame_camera forms the rays inside the refill, ngp_render_frames_camera renders a short trajectory through the scene in ONE launch
    (corner -> centre -> in_solid -> away: an expensive, an inside and an empty frame share the drain): both give, bit for bit, the frame of the same
    camera's rays in memory (ngp_get_rays), 33 x 33 included for the single camera."""
    from ngp import workload as W
    from ngp.nav import get_rays_native
    ren = constant(2.0) if kind == "constant" else real(2.0)[1]
    names = ("corner", "centre", "in_solid", "away")
    failures = []
    for res in (EVEN, ODD):
        intr = W.intrinsics(res, res)
        singles = []
        for name in names:
            pose = FP.pose(name)
            o, d = get_rays_native(pose.tolist(), intr, res, res, device=dev)
            o_np, d_np = FP.rays(name, res)
            assert np.array_equal(o.cpu().numpy(), o_np) and float(np.max(np.abs(d.cpu().numpy() - d_np))) < 1e-6
            base, _ = _frame(ren, o, d, res, dev)
            _written(base, f"{name} {res} rays in memory")
            cam = ren.render_fused_camera(pose, intr, res, res, bg_color=1)
            failures += [f"{res}x{res} {name} camera: {line}" for line in _differences(cam, base)]
            singles.append(base)
        if res % 8:
            continue                                                        # several frames per launch need multiples of 8
        many = ren.render_fused_cameras(np.stack([FP.pose(name) for name in names]), intr, res, res, bg_color=1)
        total = torch.zeros(3, dtype=torch.int64, device=dev)
        for k, name in enumerate(names):
            frame = dict(image=many["image"][k], depth=many["depth"][k], weights_sum=many["weights_sum"][k], stats=singles[k]["stats"])
            failures += [f"{res}x{res} frame {k} ({name}) of the trajectory: {line}" for line in _differences(frame, singles[k])]
            total += singles[k]["stats"][:3].to(torch.int64)
        assert torch.equal(many["stats"][:3].to(torch.int64), total), (many["stats"], total)
        assert int(singles[3]["stats"][0]) == 0 and int(total[0]) > 0       # the launch mixes an empty frame with frames that have work
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("grid_h", [4, 8, 16])
def test_small_grids_against_the_oracle(oracle, dev, grid_h):
    """density grids of 4^3 and 8^3 (fewer than 32 blocks of 4^3 a level: no coarse map, the march reads the bitfield itself) and 16^3 (a map, but neither
    block skipping nor the occupied box), from inside the scene; bars of test_gpu_fused_variants.test_other_grid_sizes"""
    from ngp import workload as W
    from ngp.field import NGPFieldFF
    from ngp.render import NGPRenderer
    bound = 2.0
    model = W.make_model(3, bound=bound)
    field = NGPFieldFF(bound=bound).to(dev).load_arrays(model)
    ren = NGPRenderer(field, bound=bound, cuda_ray=True, density_thresh=0.5, grid_size=grid_h).to(dev).eval()
    bitfield, grid = blob_bitfield(oracle, 2, grid_h, seed=2, n_blobs=40, bound=bound)
    ren.load_density_grid(grid)
    assert np.array_equal(ren.density_bitfield.cpu().numpy(), bitfield) and 0 < int(grid.sum()) < grid.size
    o, d = FP.rays("in_solid", ODD)
    ref = R.render_single_march(lambda x, dd: R.field_forward(model, x, dd, 1.0), o, d, bitfield, bound, 2, H=grid_h)
    assert ref["samples"] > 500 and int((ref["consumed"] < ref["marched"]).sum()) > 0             # rays end in these cells, some of them early
    out, ws = _frame(ren, o, d, ODD, dev)
    _written(out, f"H {grid_h}")
    assert bool((ws[FRAME_WS_HEADER:FRAME_WS_HEADER + 2 * grid_h ** 3 // 512] == 0xAB).all()) == (grid_h < 16)      # a coarse map from 16^3 on
    stats = out["stats"].cpu().numpy()
    img = out["image"].cpu().numpy()
    print(f"H {grid_h}: samples {int(stats[0])} (oracle {ref['samples']}), rays hit {int(stats[2])} (oracle {int((ref['consumed'] > 0).sum())}), "
          f"image {float(np.max(np.abs(img - ref['image']))):.2e}")
    assert abs(int(stats[0]) - ref["samples"]) <= max(8, 2e-3 * ref["samples"]) and stats[0] > 500
    assert stats[2] == int((ref["consumed"] > 0).sum())
    assert np.max(np.abs(img - ref["image"])) < 8e-3


def test_three_cascades_that_are_not_nested(oracle, dev, real):
    """bound 3.0: three cascades of half-widths 1, 2 and 3 -- the map does not fit in LDS beside the rest (no map, no skipping, no box), and the outer
    cascade's cells are not twice the middle one's.  The ring scene from its centre against the oracle; bars of test_other_grid_sizes."""
    bound = 3.0
    model, ren = real(bound)
    bitfield, cascade = FP.scene(bound)
    assert cascade == 3 and ren.cascade == 3
    o, d = FP.rays("centre", ODD)
    ref = R.render_single_march(lambda x, dd: R.field_forward(model, x, dd, 1.0), o, d, bitfield, bound, 3)
    out, ws = _frame(ren, o, d, ODD, dev)
    _written(out, "bound 3")
    assert bool((ws[FRAME_WS_HEADER:FRAME_WS_HEADER + 8192] == 0xAB).all())                         # no coarse map
    stats = out["stats"].cpu().numpy()
    img = out["image"].cpu().numpy()
    print(f"bound 3: samples {int(stats[0])} (oracle {ref['samples']}), image {float(np.max(np.abs(img - ref['image']))):.2e}")
    assert abs(int(stats[0]) - ref["samples"]) <= max(8, 2e-3 * ref["samples"]) and stats[0] > 500
    assert stats[2] == int((ref["consumed"] > 0).sum())
    assert np.max(np.abs(img - ref["image"])) < 8e-3


@pytest.mark.parametrize("grid_h", [48, 96, 127])
def test_a_grid_size_that_is_not_a_power_of_two_is_refused(dev, constant, grid_h):
    """Cells are addressed by Morton index, and for a grid size that is not a power of two the index of a cell can lie beyond H^3 (H = 48: cell
    (47, 47, 47) has index 2^18 - 1, H^3 is 110,592): the bitfield would be read past its end.  The frame kernel's launcher and the per-op marches return
    the invalid-argument code before they launch anything.  (The bitfield passed here is the 2 x 128^3 one: larger than any index these sizes can form.)"""
    import raymarching
    ren = constant(2.0)
    o, d = FP.rays("centre", ODD)
    o, d = t(o, dev), t(d, dev)
    out, _, rc = render_frame(ren, o, d, ODD, grid_size=grid_h)
    assert rc == -1 and bool(torch.isnan(out["image"]).all()) and bool((out["stats"] == -1).all())
    nears, fars = raymarching.near_far_from_aabb(o, d, ren.aabb_infer, 0.2)
    N = o.shape[0]
    with pytest.raises(RuntimeError, match="power of two"):
        raymarching.march_rays(N, 1, torch.arange(N, dtype=torch.int32, device=dev), nears.clone(), o, d, 2.0, ren.density_bitfield, 2, grid_h, nears, fars,
                               128, False, 0.0, 1024)
    with pytest.raises(RuntimeError, match="power of two"):
        raymarching.march_rays_train(o, d, 2.0, ren.density_bitfield, 2, grid_h, nears, fars, torch.zeros(2, dtype=torch.int32, device=dev), -1, False,
                                     128, True, 0.0, 1024)
