"""GPU: a frame of the default float32 field in one launch (csrc/nav_frame.hip through NGPRenderer.render_fused / render_fused_camera) against the
CPU oracle's single-march formulation over oracle.callers_oracle.DefaultField (float32, sigma times density_scale); the cases, fields and references
are tests/_default_frame_cases.py's, whose conditioning tests/test_default_frame_host.py bounds (float32 against float64: 2.4e-5 at most).

check(): image and weights_sum within 2e-4 absolute (the project's float32 tolerance for run() images, tests/test_gpu_nav_native.py: one sample
more or less at the T < 1e-4 stop moves a pixel by at most 1e-4, rounding adds ~1e-5); depth within 2e-4 * far / (far - near) per ray where the
oracle's depth is finite (a ray with far <= near has no such bound: its depth is the oracle's number), equal NaN masks; stats[2] exact; |stats[0] - samples| <= max(8, 3e-4 * samples) (tests/test_gpu_fused_variants.py).

Measured maxima on an MI355X over all cases (check() prints each case's figures before it asserts; run with -s): image 2.4e-7, weights_sum 1.2e-7,
depth 8.5e-4 of its per-ray bound, stats[0] equal to the oracle's sample count in every case, stats[2] equal; against run_cuda: image 1.8e-7,
weights_sum 0."""
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _default_frame_cases as DC  # noqa: E402

_FIELDS = {}


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def field_on(dev, which, bound):
    key = (which, bound)
    if key not in _FIELDS:
        _FIELDS[key] = DC.product_field(which, bound, dev).eval()
    return _FIELDS[key]


def renderer(dev, oracle, case, field=None, **kw):
    """NGPRenderer(cuda_ray=True) over the case's field with the case's occupancy loaded; the bitfield is the one the oracle marches"""
    from ngp.render import NGPRenderer
    field = field_on(dev, case["field"], case["bound"]) if field is None else field
    grid, bitfield, cascades = DC.occupancy(case, oracle)
    thresh = 0.5 if case["occupancy"] == "blobs" else 10.0
    ren = NGPRenderer(field, bound=case["bound"], cuda_ray=True, density_thresh=thresh, density_scale=case["density_scale"], **kw).to(dev).eval()
    assert ren.cascade == cascades
    if grid is None:
        ren.density_bitfield.fill_(255)
    else:
        ren.load_density_grid(grid)
    assert np.array_equal(ren.density_bitfield.cpu().numpy(), bitfield)
    return ren


def render(ren, case, dev, **kw):
    o, d = case["rays"]
    args = dict(dt_gamma=case["dt_gamma"], bg_color=case["bg"], max_steps=case["max_steps"], image_width=case["image_width"])
    args.update(kw)
    return ren.render_fused(t(o, dev)[None], t(d, dev)[None], **args)


def check(out, ref, case, oracle, label="", min_near=0.2):
    """min_near: the one the frame and the reference were rendered with (the depth bar is per ray, from its near and far)"""
    o, d = case["rays"]
    b = case["bound"]
    nears, fars = oracle.near_far_from_aabb(np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), np.array([-b] * 3 + [b] * 3, np.float32), min_near)
    stats = out["stats"].cpu().numpy()
    img = out["image"].reshape(-1, 3).cpu().numpy()
    ws = out["weights_sum"].cpu().numpy()
    depth = out["depth"].reshape(-1).cpu().numpy()
    finite = np.isfinite(ref["depth"])
    with np.errstate(invalid="ignore", divide="ignore"):
        depth_bound = 2e-4 * fars / (fars - nears)
    d_img, d_ws = float(np.max(np.abs(img - ref["image"]))), float(np.max(np.abs(ws - ref["weights_sum"])))
    # a ray that starts on the box's wall and leaves it at once has far <= near: no interval to march, and no per-ray bound (it would be zero or
    # negative).  Its depth is max(0 - near, 0) / (far - near), one operation on the inputs: it has to be the reference's number.
    marching = finite & (fars > nears)
    assert np.array_equal(depth[finite & ~marching], ref["depth"][finite & ~marching]), label
    d_depth = float(np.max(np.abs(depth[marching] - ref["depth"][marching]) / depth_bound[marching])) if marching.any() else 0.0
    print(f"{label}: image {d_img:.3g} weights_sum {d_ws:.3g} depth {d_depth:.3g} of its bound, samples {int(stats[0])} / {ref['samples']}, stats {stats.tolist()}")
    assert d_img < 2e-4 and d_ws < 2e-4
    assert np.array_equal(np.isnan(depth), np.isnan(ref["depth"])) and np.array_equal(np.isfinite(depth), finite)
    assert d_depth < 1.0
    assert int(stats[2]) == int((ref["consumed"] > 0).sum())
    assert abs(int(stats[0]) - ref["samples"]) <= max(8, 3e-4 * ref["samples"]), (stats, ref["samples"])
    assert int(stats[3]) >= int(stats[0])
    return stats


@pytest.mark.parametrize("name", ["two_cascades", "one_cascade", "dt_gamma_128", "dt_gamma_32", "odd_count_rgb_background", "random_field",
                                  "random_field_scale_8", "random_field_full_grid", "density_scale_2", "three_cascades", "inside_centre", "one_ray",
                                  "sixty_five_rays"])
def test_frame_against_the_oracle(oracle, dev, name):
    """cases 1-3, 5, 9-12 and 14 of the issue's table (the first one to run fails on the parent commit: NGPField has no fused_state)"""
    case = DC.CASES[name]()
    ref = DC.reference32(name)
    assert ref["samples"] > (1000 if case["rays"][0].shape[0] > 100 else 0)
    stats = check(render(renderer(dev, oracle, case), case, dev), ref, case, oracle, name)
    if case["max_steps"] == 1024:
        assert int(stats[1]) == 0


def test_sample_cap_is_counted(oracle, dev):
    case = DC.CASES["sample_cap"]()
    ref = DC.reference32("sample_cap")
    stats = check(render(renderer(dev, oracle, case), case, dev), ref, case, oracle, "sample_cap")
    assert int(ref["marched"].max()) == 64                       # the oracle's march stopped at the cap for some rays ...
    assert int(stats[1]) > 0                                     # ... and the kernel reports rays that were cut short


def test_traversal_hint_changes_nothing(oracle, dev):
    case = DC._case("A", 2.0, DC.orbit_rays(6, 48))
    ren = renderer(dev, oracle, case)
    a, b = render(ren, case, dev, image_width=48), render(ren, case, dev, image_width=0)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["depth"].nan_to_num(), b["depth"].nan_to_num())
    assert torch.equal(a["weights_sum"], b["weights_sum"]) and torch.equal(a["stats"][:3], b["stats"][:3])
    assert int(a["stats"][0]) > 1000


def test_repeatable_bit_for_bit(oracle, dev):
    """no float atomics on the data path: two launches of the same frame are identical"""
    case = DC._case("A", 2.0, DC.orbit_rays(4, 64), image_width=64)
    ren = renderer(dev, oracle, case)
    a, b = render(ren, case, dev), render(ren, case, dev)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["weights_sum"], b["weights_sum"]) and torch.equal(a["depth"].nan_to_num(), b["depth"].nan_to_num())
    assert torch.equal(a["stats"][:3], b["stats"][:3]) and int(a["stats"][0]) > 1000


@pytest.mark.parametrize("hw", [(40, 40), (24, 56)])
def test_camera_mode_is_get_rays_then_the_frame(oracle, dev, hw):
    from ngp import nav
    from ngp import workload as W
    H, Wd = hw
    case = DC._case("A", 2.0, DC.orbit_rays(2, 8))
    ren = renderer(dev, oracle, case)
    pose, intr = W.orbit_pose(5), W.intrinsics(H, Wd)
    cam = ren.render_fused_camera(pose, intr, H, Wd, bg_color=DC.BG)
    o, d = nav.get_rays_native(pose, intr, H, Wd, device=dev)
    rays = ren.render_fused(o, d, bg_color=DC.BG, image_width=Wd)
    assert cam["image"].shape == (H, Wd, 3) and cam["depth"].shape == (H, Wd) and cam["weights_sum"].shape == (H * Wd,)
    assert torch.equal(cam["image"].reshape(-1, 3), rays["image"]) and torch.equal(cam["weights_sum"], rays["weights_sum"])
    assert torch.equal(cam["depth"].reshape(-1).nan_to_num(), rays["depth"].nan_to_num()) and torch.equal(cam["stats"][:3], rays["stats"][:3])
    assert int(cam["stats"][0]) > 1000


def test_no_samples_at_all(oracle, dev):
    case = DC.CASES["inside_away"]()
    assert DC.reference32("inside_away")["samples"] == 0
    out = render(renderer(dev, oracle, case), case, dev, bg_color=DC.BG)
    stats = out["stats"].cpu().numpy()
    assert torch.equal(out["image"].reshape(-1, 3), t(np.array(DC.BG, np.float32), dev).expand(out["weights_sum"].shape[0], 3))
    assert float(out["weights_sum"].abs().max()) == 0.0 and int(stats[0]) == 0 and int(stats[2]) == 0 and int(stats[3]) == 0


def test_against_the_op_by_op_route(oracle, dev):
    """the same frame through run_cuda in eval mode: the product's own occupancy-grid route, launch by launch"""
    case = DC.CASES["two_cascades"]()
    ren = renderer(dev, oracle, case)
    o, d = case["rays"]
    out = render(ren, case, dev)
    with torch.no_grad():
        perop = ren.run_cuda(t(o, dev)[None], t(d, dev)[None], bg_color=1)
    d_img = float((out["image"] - perop["image"]).abs().max())
    d_ws = float((out["weights_sum"] - perop["weights_sum"]).abs().max())
    print(f"run_cuda: image {d_img:.3g} weights_sum {d_ws:.3g}")
    assert d_img < 2e-4 and d_ws < 2e-4


def test_a_changed_weight_reaches_the_next_frame(oracle, dev):
    """the prepared (transposed) weights are redone when a parameter changes in place"""
    from _util import oracle_field
    case = DC.CASES["two_cascades"]()
    field = DC.product_field("A", 2.0, dev).eval()               # a copy of its own: the shared field stays as it is
    ren = renderer(dev, oracle, case, field=field)
    before = render(ren, case, dev)
    with torch.no_grad():
        field.color_net[2].weight.mul_(0.5)
    after = render(ren, case, dev)
    assert float((after["image"] - before["image"]).abs().max()) > 1e-2
    check(after, DC.reference("two_cascades", oracle, field=oracle_field(field)), case, oracle, "changed weight")


def test_refusals_name_their_reason(oracle, dev):
    from ngp import workload as W
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    case = DC.CASES["one_ray"]()
    o, d = (t(a, dev)[None] for a in case["rays"])
    with_bg = NGPRenderer(NGPField(bound=2.0, bg_radius=3.0).to(dev), bound=2.0, cuda_ray=True, bg_radius=3.0).to(dev).eval()
    with pytest.raises(ValueError, match="bg_radius"):
        with_bg.render_fused(o, d)
    with pytest.raises(ValueError, match="bg_radius"):
        with_bg.render_fused_camera(W.orbit_pose(0), W.intrinsics(8, 8), 8, 8)
    no_grid = NGPRenderer(field_on(dev, "A", 2.0), bound=2.0, cuda_ray=False).to(dev).eval()
    with pytest.raises(ValueError, match="cuda_ray=False"):
        no_grid.render_fused(o, d)
    wide = NGPRenderer(NGPField(bound=2.0, num_layers=3).to(dev), bound=2.0, cuda_ray=True).to(dev).eval()
    with pytest.raises(ValueError, match="default float32 NGPField"):
        wide.render_fused(o, d)
    ren = renderer(dev, oracle, case)
    with pytest.raises(ValueError, match="render_fused_camera"):
        ren.render_fused_cameras(np.stack([W.orbit_pose(0), W.orbit_pose(1)]), W.intrinsics(8, 8), 8, 8)
